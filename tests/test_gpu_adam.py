"""GPU: the fused Adam step (`node_adam_step` through the C ABI, optim.FusedAdam) against torch.optim.Adam -- the
reference's `-o adam` (train.py:138) -- element by element with an fp64 arbiter, its device-side step counters, the skip
flag, state interchange with torch.optim.Adam, deferred completion and the training CLI.

The accuracy rule, for p, exp_avg and exp_avg_sq after every step:

    max|fused - fp64| <= 4 * max|torch_fp32 - fp64| + 1 ulp of max|fp64|

The yardstick is PyTorch's own fp32 Adam on the same inputs (CPU), the arbiter PyTorch's Adam in fp64.  The factor 4 covers
operation order (FMA contraction; a * m + (1 - a) * g against lerp), the ulp the case where PyTorch's fp32 result happens to be
exact.  The maxima run over one tensor where it has 257 elements or more, and over the smaller tensors of one launch of the
table (64 consecutive tensors of the group) together: the largest fp32 error PyTorch makes on the 8 elements of one tensor is
a matter of luck (a fifth of an ulp as easily as a whole one), not a yardstick.  The first test prints the measured ratios (fused error over PyTorch's fp32 error); on an
MI355X, worst case of the 10 steps: p 1.51, exp_avg 1.47, exp_avg_sq 1.00 at (lr 0.1, wd 1e-4) and p 1.00, exp_avg 2.16,
exp_avg_sq 1.00 at (lr 1e-3, wd 0).
"""
import copy
import csv
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = 'cuda'
KEYS = ('exp_avg', 'exp_avg_sq')


def _ulp(x):
    """One fp32 unit in the last place at |x|."""
    x = torch.tensor(abs(float(x)), dtype=torch.float32)
    return float(torch.nextafter(x, torch.tensor(float('inf'))) - x)


def _flat(tensors):
    """One host copy of a list of tensors, in fp64."""
    return torch.cat([t.detach().reshape(-1) for t in tensors]).cpu().double()


def _quantities(opt, params):
    """{'p' | 'exp_avg' | 'exp_avg_sq': flat fp64 host copy over `params`}; a parameter that has no state yet counts as zeros."""
    out = {'p': _flat(params)}
    for k in KEYS:
        out[k] = _flat([opt.state[p][k] if k in opt.state[p] else torch.zeros_like(p) for p in params])
    return out


def _hold(fused, yard, arbiter, sizes, label, ratios=None):
    """The rule of the module docstring.  `ratios` collects the worst error ratio per quantity (for the figures in DESIGN.md)."""
    starts = [sum(sizes[:i]) for i in range(len(sizes))]
    cases = [('tensor %d (n = %d)' % (i, n), [i]) for i, n in enumerate(sizes) if n >= 257]
    for first in range(0, len(sizes), 64):      # the smaller tensors of one launch of the table together
        small = [i for i in range(first, min(first + 64, len(sizes))) if sizes[i] < 257]
        if small:
            cases.append(('the %d tensors below 257 elements among tensors %d..%d' % (len(small), first, first + 63), small))
    for k in ('p',) + KEYS:
        for name, members in cases:
            f, y, a = (torch.cat([q[k][starts[i]:starts[i] + sizes[i]] for i in members]) for q in (fused, yard, arbiter))
            err, ref = float((f - a).abs().max()), float((y - a).abs().max())
            bound = 4.0 * ref + _ulp(a.abs().max())
            if ratios is not None and ref > 0:
                ratios[k] = max(ratios.get(k, 0.0), err / ref)
            assert err <= bound, '%s: %s of %s: |fused - fp64| %.3e > 4 * %.3e + ulp = %.3e' % (label, k, name, err, ref, bound)


class Trio:
    """The same parameters three times -- FusedAdam on the GPU, torch.optim.Adam in fp32 and in fp64 on the CPU -- fed the same
    gradients.  `odd` names the tensors whose GPU gradient sits at an odd float offset of a shared buffer (the unaligned path)."""

    def __init__(self, sizes, lr, wd, seed, odd=()):
        import neural_ode_features_amd as nof
        self.sizes, self.odd = list(sizes), set(odd)
        self.gen = torch.Generator().manual_seed(seed)
        init = [torch.randn(n, generator=self.gen) for n in self.sizes]
        self.pg = [t.to(DEV, copy=True).requires_grad_(True) for t in init]
        self.p32 = [t.clone().requires_grad_(True) for t in init]
        self.p64 = [t.double().requires_grad_(True) for t in init]
        self.og = nof.FusedAdam(self.pg, lr=lr, weight_decay=wd)
        self.o32 = torch.optim.Adam(self.p32, lr=lr, weight_decay=wd)
        self.o64 = torch.optim.Adam(self.p64, lr=lr, weight_decay=wd)
        self.shared = torch.zeros(sum(self.sizes[i] + 1 for i in self.odd) + 1, device=DEV)

    def gradients(self):
        """randn * 10 ** randint(-3, 2) per element: magnitudes over five decades inside one tensor."""
        return [torch.randn(n, generator=self.gen) * 10.0 ** torch.randint(-3, 3, (n,), generator=self.gen).float() for n in self.sizes]

    def give(self, grads):
        off = 1
        for i, g in enumerate(grads):
            if g is None:
                self.pg[i].grad = self.p32[i].grad = self.p64[i].grad = None
                continue
            if i in self.odd:
                view = self.shared[off:off + g.numel()]
                assert view.data_ptr() % 16 != 0 and view.data_ptr() % 4 == 0
                view.copy_(g)
                off += g.numel() + g.numel() % 2                          # the next offset is odd again
                self.pg[i].grad = view
            else:
                self.pg[i].grad = g.to(DEV)
            self.p32[i].grad, self.p64[i].grad = g.clone(), g.double()

    def step(self, grads):
        self.give(grads)
        for o in (self.og, self.o32, self.o64):
            o.step()

    def hold(self, label, ratios=None):
        _hold(_quantities(self.og, self.pg), _quantities(self.o32, self.p32), _quantities(self.o64, self.p64), self.sizes, label, ratios)


# the kernel's seams: scalar path only (1, 3), vector path without and with a tail (4, 5, 257, 1023), fewer elements than
# threads, more than one grid-stride trip of the vector path plus a tail (65543 = 4 * (64 * 256) + 7), a gradient off the
# 16-byte grid, and 150 small tensors that make the table travel in three launches
SEAM_SIZES = [1, 3, 4, 5, 257, 1023, 65543, 1001] + [8] * 150
ODD = (7,)


@pytest.mark.parametrize('lr,wd', [(0.1, 1e-4), (1e-3, 0.0)])
def test_fused_adam_element_by_element_against_the_fp64_arbiter(lr, wd):
    trio = Trio(SEAM_SIZES, lr, wd, seed=11, odd=ODD)
    assert len(SEAM_SIZES) > 2 * 64
    ratios = {}
    for step in range(10):
        trio.step(trio.gradients())
        trio.hold('lr %g wd %g step %d' % (lr, wd, step + 1), ratios)
    print('fused Adam error over torch fp32 error (worst case of 10 steps), lr %g wd %g: %s'
          % (lr, wd, '  '.join('%s %.2f' % (k, ratios[k]) for k in ('p',) + KEYS)))
    assert all(float(trio.og.state[p]['step']) == 10.0 for p in trio.pg)
    assert all(trio.og.state[p]['step'].device == p.device and trio.og.state[p]['step'].dtype == torch.float32 for p in trio.pg)


def test_tensors_whose_step_counts_differ():
    """A parameter without a gradient is skipped and its counter stands still (torch.optim.Adam does the same): the bias
    corrections are per tensor.  All-zero gradients without weight decay change nothing: 0 / (0 + eps) = 0."""
    trio = Trio([257, 1023, 64, 300], lr=1e-3, wd=0.0, seed=12)
    start = trio.pg[3].detach().clone()
    for step in range(1, 6):
        grads = trio.gradients()
        if step in (2, 3):
            grads[1] = None
        grads[3] = torch.zeros(300)
        trio.step(grads)
        trio.hold('step %d' % step)
    counts = [float(trio.og.state[p]['step']) for p in trio.pg]
    assert counts == [5.0, 3.0, 5.0, 5.0]
    assert counts == [float(trio.o32.state[p]['step']) for p in trio.p32]
    assert torch.equal(trio.pg[3], start)
    assert not trio.og.state[trio.pg[3]]['exp_avg'].any() and not trio.og.state[trio.pg[3]]['exp_avg_sq'].any()


def _pair(sizes, seed, **kw):
    """Two FusedAdam instances over identical GPU parameters, and a gradient source."""
    import neural_ode_features_amd as nof
    gen = torch.Generator().manual_seed(seed)
    init = [torch.randn(n, generator=gen) for n in sizes]
    pa = [t.to(DEV, copy=True).requires_grad_(True) for t in init]
    pb = [t.to(DEV, copy=True).requires_grad_(True) for t in init]

    def grads():
        return [(torch.randn(n, generator=gen) * 10.0 ** torch.randint(-3, 3, (n,), generator=gen).float()).to(DEV) for n in sizes]

    return pa, pb, nof.FusedAdam(pa, **kw), nof.FusedAdam(pb, **kw), grads


def _state(opt, params):
    return [t.detach().clone() for p in params for t in (p, opt.state[p]['exp_avg'], opt.state[p]['exp_avg_sq'], opt.state[p]['step'])]


def _same(opt_a, pa, opt_b, pb):
    return all(torch.equal(x, y) for x, y in zip(_state(opt_a, pa), _state(opt_b, pb)))


def test_skip_flag_commits_nothing_and_counts_nothing():
    sizes = [5, 257, 4099] + [8] * 70
    pa, pb, oa, ob, grads = _pair(sizes, 13, lr=1e-2, weight_decay=1e-4)
    for _ in range(2):
        g = grads()
        for p, q, t in zip(pa, pb, g):
            p.grad, q.grad = t, t.clone()
        oa.step()
        ob.step()
    assert _same(oa, pa, ob, pb)
    flag, other = torch.ones(1, device=DEV), torch.full((1,), 3.0, device=DEV)
    oa.skip_flag, oa.flags_to_reset = flag, [flag, other]
    before = _state(oa, pa)
    for p, t in zip(pa, grads()):
        p.grad = t
    oa.step()                                                # skipped on the device: the twin never sees this call
    assert all(torch.equal(x, y) for x, y in zip(before, _state(oa, pa)))
    assert all(float(oa.state[p]['step']) == 2.0 for p in pa)
    assert float(flag) == 0.0 and float(other) == 0.0
    g = grads()
    for p, q, t in zip(pa, pb, g):
        p.grad, q.grad = t, t.clone()
    oa.step()                                                # the flag reads 0 now: committed
    ob.step()
    assert _same(oa, pa, ob, pb)
    assert all(float(oa.state[p]['step']) == 3.0 for p in pa)
    assert not all(torch.equal(x, y) for x, y in zip(before, _state(oa, pa)))


def test_grad_scale_is_folded_into_the_step():
    """grad_scale = 0.5 over doubled gradients is the plain step bit for bit: powers of two are exact."""
    pa, pb, oa, ob, grads = _pair([3, 257, 4099], 14, lr=1e-2, weight_decay=1e-4)
    oa.grad_scale = 0.5
    for _ in range(3):
        for p, q, t in zip(pa, pb, grads()):
            p.grad, q.grad = 2.0 * t, t
        oa.step()
        ob.step()
        assert _same(oa, pa, ob, pb)


def test_state_loads_into_torch_adam():
    """Three fused steps, then torch.optim.Adam over a twin on the GPU takes the state over and both go on: they stay together
    within the rule, against an fp64 twin on the CPU that saw every gradient."""
    trio = Trio([5, 257, 4099], lr=1e-2, wd=1e-4, seed=15)
    for _ in range(3):
        trio.step(trio.gradients())
    twin = [p.detach().clone().requires_grad_(True) for p in trio.pg]
    ot = torch.optim.Adam(twin, lr=1e-2, weight_decay=1e-4)
    ot.load_state_dict(copy.deepcopy(trio.og.state_dict()))          # (a copy: the two must not step the same moment tensors)
    assert all(float(ot.state[p]['step']) == 3.0 for p in twin)
    for step in range(2):
        grads = trio.gradients()
        trio.step(grads)
        for p, g in zip(twin, grads):
            p.grad = g.to(DEV)
        ot.step()
        _hold(_quantities(trio.og, trio.pg), _quantities(ot, twin), _quantities(trio.o64, trio.p64), trio.sizes, 'after the hand-over, step %d' % (step + 1))
    assert all(float(ot.state[p]['step']) == 5.0 for p in twin)


def test_torch_adam_state_from_the_cpu_loads_and_its_count_is_used():
    """What a checkpoint of the reference holds: torch.optim.Adam's state with `step` as a 0-d CPU tensor.  The next fused
    step moves the count to the device and forms its bias corrections from it (from a count of 0 the update would be 3.4 times
    as large)."""
    import neural_ode_features_amd as nof
    sizes = [5, 257, 4099]
    trio = Trio(sizes, lr=1e-2, wd=1e-4, seed=16)
    for _ in range(3):
        grads = trio.gradients()
        trio.give(grads)
        trio.o32.step()
        trio.o64.step()
    pg = [p.detach().clone().to(DEV).requires_grad_(True) for p in trio.p32]
    og = nof.FusedAdam(pg, lr=0.5)                                    # the loaded group brings lr and weight decay
    og.load_state_dict(copy.deepcopy(trio.o32.state_dict()))
    assert all(og.state[p]['step'].device.type == 'cpu' and og.state[p]['step'].dim() == 0 for p in pg)
    assert og.param_groups[0]['lr'] == 1e-2 and og.param_groups[0]['weight_decay'] == 1e-4
    grads = trio.gradients()
    trio.give(grads)
    trio.o32.step()
    trio.o64.step()
    for p, g in zip(pg, grads):
        p.grad = g.to(DEV)
    og.step()
    assert all(og.state[p]['step'].device == p.device and float(og.state[p]['step']) == 4.0 for p in pg)
    _hold(_quantities(og, pg), _quantities(trio.o32, trio.p32), _quantities(trio.o64, trio.p64), sizes, 'first step on the loaded state')
    # a plain number for a count (older torch versions stored one) is taken the same way
    for p in pg:
        og.state[p]['step'] = 4
    for p, g in zip(pg, trio.gradients()):
        p.grad = g.to(DEV)
    og.step()
    assert all(torch.is_tensor(og.state[p]['step']) and float(og.state[p]['step']) == 5.0 for p in pg)


def test_adam_step_argument_checks():
    from neural_ode_features_amd import _lib
    lib = _lib.load()
    t = torch.zeros(64, device=DEV)
    a = t.data_ptr()
    Row = _lib.NodeAdamTensor

    def call(row, count=1, lr=0.1, b1=0.9, b2=0.999, eps=1e-8, wd=0.0):
        return lib.node_adam_step((Row * 1)(row) if row is not None else None, count, lr, b1, b2, eps, wd, 1.0, None, None)

    good = Row(a, a + 64, a + 128, a + 192, a + 252, 8)
    assert call(None) == -1
    for k in range(5):                                                # a NULL in any pointer field
        fields = [a, a + 64, a + 128, a + 192, a + 252, 8]
        fields[k] = None
        assert call(Row(*fields)) == -1, k
    assert call(Row(a + 2, a + 64, a + 128, a + 192, a + 252, 8)) == -9
    assert call(Row(a, a + 64, a + 128, a + 192, a + 254, 8)) == -9
    assert call(good, lr=-0.1) == -9
    assert call(good, eps=-1e-8) == -9 and call(good, wd=-0.1) == -9
    assert call(good, b1=1.0) == -9 and call(good, b2=1.0) == -9 and call(good, b1=-0.1) == -9
    assert call(good, count=-1) == -9
    assert call(good, count=0) == 0 and call(None, count=0) == 0
    torch.cuda.synchronize()
    assert not t.any()                                                # no refused call launched anything
    assert call(good) == 0                                            # ... and the record itself is a good one
    torch.cuda.synchronize()
    assert float(t[63]) == 1.0 and not t[:63].any()                   # zero gradients, no decay: only the counter moved


def _block(seed=7, tol=1e-4):
    """The block of tests/test_gpu_deferred.py::_block."""
    import neural_ode_features_amd as nof
    from tests.helpers import make_func
    f, _ = make_func(32, seed=seed, device='cuda', kink_free=True)
    blk = nof.ODEBlock(n_filters=32, tol=tol, method='dopri5', adjoint=True, t1=1)
    blk.odefunc.load_state_dict(f.state_dict())
    return blk.cuda()


def _adam_pair():
    import neural_ode_features_amd as nof
    a = _block()
    b = copy.deepcopy(a)
    # lr 1e-4: Adam moves every weight by about lr per step whatever its gradient; steps this small keep the solver's step
    # counts from jumping by two between iterations (a jump by one is covered by the spare step), which would be a miss
    return a, b, nof.FusedAdam(a.parameters(), lr=1e-4, weight_decay=1e-4), nof.FusedAdam(b.parameters(), lr=1e-4, weight_decay=1e-4)


def test_deferred_adam_steps_equal_synchronous_steps():
    from neural_ode_features_amd import integrate
    a, b, oa, ob = _adam_pair()
    x = torch.randn(4, 32, 8, 8, generator=torch.Generator().manual_seed(1)).cuda()
    d = integrate.Deferred(x.device)
    oa.use_deferred(d)
    with d:
        for _ in range(4):
            a(x).square().mean().backward()
            oa.step()
            oa.zero_grad()
    for _ in range(4):
        b(x).square().mean().backward()
        ob.step()
        ob.zero_grad()
    assert d.resolve() == 0 and d.blind_solves == 6
    assert _same(oa, list(a.parameters()), ob, list(b.parameters()))
    assert all(float(oa.state[p]['step']) == 4.0 for p in a.parameters())


def test_deferred_loop_repeats_a_missed_adam_batch_and_counts_every_batch_once():
    """integrate.DeferredLoop with FusedAdam: the sixth of eight batches is enqueued with ONE step (a certain miss, forced as
    tests/test_gpu_deferred.py forces it).  Its update and the one behind it are skipped on the device -- counters included --
    and both batches are repeated: parameters, moments and counters equal the synchronous run bit for bit."""
    from neural_ode_features_amd import integrate
    a, b, oa, ob = _adam_pair()
    gen = torch.Generator().manual_seed(11)
    xs = [torch.randn(4, 32, 8, 8, generator=gen).cuda() for i in range(8)]

    def make_step(blk, opt):
        def step(x):
            loss = F.dropout(blk(x), 0.5, training=True).square().mean()
            loss.backward()
            opt.step()
            opt.zero_grad()
            return loss.detach()
        return step

    torch.manual_seed(3)
    torch.cuda.manual_seed(3)
    sync_step = make_step(b, ob)
    losses_b = [sync_step(x) for x in xs]

    torch.manual_seed(3)
    torch.cuda.manual_seed(3)
    d = integrate.Deferred(xs[0].device)
    loop = integrate.DeferredLoop(d, oa, make_step(a, oa))
    losses_a = []
    for i, x in enumerate(xs):
        if i == 5:
            d.resolve()
            d.force_counts(1)
        losses_a += loop.step(x)
    losses_a += loop.flush()
    assert len(losses_a) == 8
    assert (loop.retries, loop.miss_events) == (2, 1) and d.misses >= 1, (loop.retries, loop.miss_events, d.misses)
    for i, (la, lb) in enumerate(zip(losses_a, losses_b)):
        assert float(la) == float(lb), i
    assert _same(oa, list(a.parameters()), ob, list(b.parameters()))
    assert all(float(oa.state[p]['step']) == 8.0 for p in a.parameters())       # no skipped launch advanced a counter
    assert float(d.miss_flag) == 0.0


def test_train_cli_with_adam_under_deferred_completion_and_resume(tmp_path):
    import neural_ode_features_amd as nof
    from neural_ode_features_amd import train as T
    run = str(tmp_path / 'run')
    common = ['-o', 'adam', '--deferred', '-a', '--dataset', 'mnist', '-f', '16', '--synthetic-size', '64', '-b', '32',
              '--lr', '1e-3', '--lrschedule', 'fixed', '--run-dir', run]
    assert T.main(common + ['-e', '2']) == 0
    assert [int(r['epoch']) for r in csv.DictReader(open(os.path.join(run, 'log.csv')))] == [1, 2]
    ck = torch.load(os.path.join(run, 'last.pth'), map_location='cpu', weights_only=False)
    st = ck['optim']['state']
    assert ck['epoch'] == 2 and st and all('exp_avg' in v and 'exp_avg_sq' in v for v in st.values())
    assert all(float(v['step']) == 4.0 for v in st.values())          # 2 epochs of 2 batches, each counted once
    assert ck['optim']['param_groups'][0]['betas'] == (0.9, 0.999) and ck['optim']['param_groups'][0]['lr'] == 1e-3
    # torch.optim.Adam's layout: the reference's optimizer takes this checkpoint
    net = nof.ODENet(1, out=10, n_filters=16, adjoint=True)
    torch.optim.Adam(net.parameters(), lr=0.1).load_state_dict(ck['optim'])
    assert T.main(common + ['-e', '3', '--resume']) == 0
    assert [int(r['epoch']) for r in csv.DictReader(open(os.path.join(run, 'log.csv')))] == [1, 2, 3]
    ck3 = torch.load(os.path.join(run, 'last.pth'), map_location='cpu', weights_only=False)
    assert ck3['epoch'] == 3 and all(float(v['step']) == 6.0 for v in ck3['optim']['state'].values())   # the counts went on from 4

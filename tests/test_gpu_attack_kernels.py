"""GPU: the attack's per-iteration kernels (csrc/kernels_attack.hip: node_attack_step, node_attack_judge) against the plain-torch
loop's single step (neural_ode_features_amd/attack.py: step_reference, distance_reference) run in fp64 on the CPU.

Bounds: the L-infinity update is sign, multiply by representable factors, add and clamp -- the kernel performs the very fp32
operations of the fp32 torch statement, so the new x is compared BIT FOR BIT with it.  The L2 update and the normalised output
are compared with fp64 at 1e-6 absolute: about eight fp32 roundings of 6e-8 on values in [0, 1] (the normalised output: the
x error divided by std ~ 0.2 plus two roundings of a value of magnitude <= 2.6)."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

INF = float('inf')
MEAN3, STD3 = (0.4914, 0.4822, 0.4465), (0.2023, 0.1994, 0.2010)
SHAPES = [(5, 3, 32, 32), (3, 1, 28, 28), (2, 3, 5, 7)]       # 105 elements: tails in every reduction
ROLES = ('outside', 'inactive', 'zero', 'inside')
SETTINGS = {INF: dict(epsilon=0.03, stepsize=0.01), 2: dict(epsilon=0.05, stepsize=0.02)}


def _inputs(shape, shift, seed):
    """x0, x, g, active with, by sample, the roles ROLES[(i + shift) % 4]: outside the eps-ball, inactive, an all-zero gradient,
    inside the ball; every sample has pixels at both bounds (in x0 and in x)."""
    n = shape[0]
    gen = torch.Generator().manual_seed(seed)
    x0 = torch.rand(shape, generator=gen)
    x0.flatten(1)[:, 0::11] = 0.0
    x0.flatten(1)[:, 1::11] = 1.0
    g = torch.randn(shape, generator=gen) * 1e-3
    x = x0.clone()
    active = torch.ones(n, dtype=torch.int32)
    roles = [ROLES[(i + shift) % 4] for i in range(n)]
    for i, role in enumerate(roles):
        noise = torch.rand(shape[1:], generator=gen) * 2 - 1
        if role == 'outside':
            x[i] = (x0[i] + 0.2 * noise).clamp(0, 1)
        elif role == 'inside':
            x[i] = (x0[i] + 1e-3 * noise).clamp(0, 1)
        elif role == 'zero':
            x[i] = (x0[i] + 1e-2 * noise).clamp(0, 1)
            g[i] = 0.0
        else:
            x[i] = (x0[i] + 0.1 * noise).clamp(0, 1)
            active[i] = 0
    return x0, x, g, active, roles


def _attack_struct(shape, norm, epsilon, stepsize, return_early, stats):
    from neural_ode_features_amd import _lib
    n, c, h, w = shape
    return _lib.NodeAttack(n, c, h, w, _lib.ATTACK_LINF if norm == INF else _lib.ATTACK_L2, int(return_early), stepsize, epsilon, 0.0, 1.0,
                           stats[0].data_ptr() if stats else None, stats[1].data_ptr() if stats else None)


def _run_step(shape, norm, x0, x, g, active, pre):
    from neural_ode_features_amd import _lib
    lib = _lib.load()
    stats = None
    if pre is not None:
        stats = (torch.tensor(pre[0], dtype=torch.float32, device='cuda'), torch.tensor(pre[1], dtype=torch.float32, device='cuda'))
    atk = _attack_struct(shape, norm, SETTINGS[norm]['epsilon'], SETTINGS[norm]['stepsize'], True, stats)
    xd, x0d, gd, ad = x.cuda(), x0.cuda(), g.cuda(), active.cuda()
    xn = torch.full(shape, 7.0, dtype=torch.float32, device='cuda')
    _lib.check(lib.node_attack_step(C.byref(atk), xd.data_ptr(), x0d.data_ptr(), gd.data_ptr(), ad.data_ptr(), xn.data_ptr(),
                                    torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return xd.cpu(), xn.cpu()


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('norm', [INF, 2], ids=['linf', 'l2'])
@pytest.mark.parametrize('pre', [True, False], ids=['normalised', 'plain'])
def test_attack_step_matches_the_torch_step(shape, norm, pre):
    from neural_ode_features_amd.attack import step_reference
    c = shape[1]
    stats = ((MEAN3[:c], STD3[:c]) if pre else None)
    seen = set()
    for shift in (0, 2):
        x0, x, g, active, roles = _inputs(shape, shift, seed=sum(shape) + shift)
        seen |= set(roles)
        got_x, got_xn = _run_step(shape, norm, x0, x, g, active, stats)
        if stats:
            mean = torch.tensor(stats[0]).reshape(1, -1, 1, 1)
            std = torch.tensor(stats[1]).reshape(1, -1, 1, 1)
        else:
            mean, std = torch.zeros(1, c, 1, 1), torch.ones(1, c, 1, 1)
        kw = SETTINGS[norm]
        # the gradient with respect to the pixels: the chain rule through (x - mean) / std
        ref64 = step_reference(x.double(), x0.double(), g.double() / std.double(), norm, kw['stepsize'], kw['epsilon'])
        ref32 = step_reference(x, x0, g / std, norm, kw['stepsize'], kw['epsilon'])
        xn64 = (ref64 - mean.double()) / std.double()
        for i, role in enumerate(roles):
            if role == 'inactive':
                assert torch.equal(got_x[i], x[i]), 'an inactive sample moved'
                assert bool((got_xn[i] == 7.0).all()), 'an inactive sample\'s model input was written'
                continue
            ex = float((got_x[i].double() - ref64[i]).abs().max())
            en = float((got_xn[i].double() - xn64[i]).abs().max())
            print('%s norm %s %s sample %d (%s): x error %.2e, normalised %.2e' % (shape, norm, 'pre' if pre else 'plain', i, role, ex, en))
            if norm == INF:
                assert torch.equal(got_x[i], ref32[i]), (role, ex)
            assert ex <= 1e-6, (role, ex)
            assert en <= 1e-6, (role, en)
            if role == 'zero':       # sign 0 / the 1e-12 clamp: the update is the projection of the old perturbation alone
                assert float((ref64[i] - x[i].double()).abs().max()) <= 1e-7
            d = (got_x[i] - x0[i]).double()
            size = float(d.abs().max()) if norm == INF else float(d.pow(2).mean().sqrt())
            assert size <= kw['epsilon'] * (1 + 1e-5)
            if role == 'outside':
                assert size >= kw['epsilon'] * 0.5
            assert float(got_x[i].min()) >= 0.0 and float(got_x[i].max()) <= 1.0
    assert seen == set(ROLES)


def _judge_ref(rec, logits, labels, x, x0, initial, iteration, norm, return_early):
    """The judge restated per sample in fp64 (rec: dict of lists, updated in place)."""
    from neural_ode_features_amd.attack import distance_reference
    dist = distance_reference(x.double(), x0.double(), norm)
    for i in range(logits.shape[0]):
        row = logits[i].tolist()
        pred = row.index(max(row))               # first index on ties
        wrong = pred != int(labels[i])
        if initial:
            rec['original'][i] = pred
            if wrong:
                rec['adv'][i], rec['found'][i], rec['dist'][i], rec['active'][i] = pred, 0, 0.0, 0
                rec['best'][i] = x[i].clone()
            continue
        if not rec['active'][i] or not wrong:
            continue
        if return_early or float(dist[i]) < rec['dist'][i]:
            rec['adv'][i], rec['found'][i], rec['dist'][i] = pred, iteration, float(dist[i])
            rec['best'][i] = x[i].clone()
            if return_early:
                rec['active'][i] = 0


@pytest.mark.parametrize('norm', [INF, 2], ids=['linf', 'l2'])
@pytest.mark.parametrize('return_early', [True, False], ids=['early', 'keep_smallest'])
@pytest.mark.parametrize('classes', [10, 300], ids=['c10', 'c300'])
def test_attack_judge_bookkeeping(norm, return_early, classes):
    """Three calls: the initial one, an iteration with moderate perturbations, one with a smaller perturbation for sample 0 and
    larger ones for the rest (without return_early only a strictly smaller distance replaces the record).  Samples: correct / natural error at the start; later fooled or not; made
    inactive by hand; ties in the logits between the label and a lower / a higher class index, within a wave and across waves."""
    from neural_ode_features_amd import _lib
    lib = _lib.load()
    shape = (8, 3, 5, 7)
    n = shape[0]
    gen = torch.Generator().manual_seed(classes + int(return_early))
    x0 = torch.rand(shape, generator=gen)
    labels = torch.tensor([3, 3, 3, 3, 5, 5, 5, 5]) + (classes - 10)

    def logits_for(winners):
        lg = torch.randn(n, classes, generator=gen)
        for i, wn in enumerate(winners):
            for j in wn:
                lg[i, j] = 9.0        # every listed class ties at the top
        return lg
    lab = int(labels[0]), int(labels[4])
    # call 0: samples 0, 1, 4, 5, 6 correct; 2 a natural error; 3 a tie label / lower index -> the lower index wins (wrong);
    # 7 a tie label / higher index -> the label wins (correct)
    w0 = [[lab[0]], [lab[0]], [0], [1, lab[0]], [lab[1]], [lab[1]], [lab[1]], [lab[1], classes - 1]]
    # call 1: 0 fooled; 1 still correct; 4 fooled through a tie across the class range; 5 fooled but made inactive by hand; 6 fooled; 7 correct
    w1 = [[7], [lab[0]], [5], [2], [0, lab[1], classes - 1], [2], [classes - 1], [lab[1]]]
    # call 2: 0 fooled again (at a smaller distance), 1 fooled now, 4 fooled (at a larger distance), 6 correct again, 7 fooled
    w2 = [[8], [0], [5], [2], [1], [2], [lab[1]], [0]]
    rec = dict(active=[1] * n, original=[-1] * n, adv=[-1] * n, found=[-1] * n, dist=[INF] * n, best=[None] * n)
    d = dict(active=torch.ones(n, dtype=torch.int32, device='cuda'), original=torch.full((n,), -1, dtype=torch.int32, device='cuda'),
             adv=torch.full((n,), -1, dtype=torch.int32, device='cuda'), found=torch.full((n,), -1, dtype=torch.int32, device='cuda'),
             dist=torch.full((n,), INF, dtype=torch.float32, device='cuda'), best=torch.full(shape, -1.0, dtype=torch.float32, device='cuda'))
    atk = _attack_struct(shape, norm, 0.1, 0.01, return_early, None)
    record = _lib.NodeAttackRecord(d['active'].data_ptr(), d['original'].data_ptr(), d['adv'].data_ptr(), d['found'].data_ptr(),
                                   d['dist'].data_ptr(), d['best'].data_ptr())
    x0d, ld = x0.cuda(), labels.cuda()
    # perturbation sizes: call 1 moderate; call 2 SMALLER for sample 0 (its record is replaced when the attack keeps the smallest), larger for the rest
    scale = {0: torch.zeros(n), 1: torch.full((n,), 0.1), 2: torch.tensor([0.02] + [0.3] * (n - 1))}
    for call, winners in enumerate((w0, w1, w2)):
        x = (x0 + (scale[call] * torch.linspace(0.5, 1.0, n)).reshape(n, 1, 1, 1) * (torch.rand(shape, generator=gen) * 2 - 1)).clamp(0, 1)
        lg = logits_for(winners)
        if call == 1:        # a sample switched off from outside stays untouched whatever it predicts
            rec['active'][5] = 0
            d['active'][5] = 0
        _judge_ref(rec, lg, labels, x, x0, call == 0, call, norm, return_early)
        xd, lgd = x.cuda(), lg.cuda()
        _lib.check(lib.node_attack_judge(C.byref(atk), classes, lgd.data_ptr(), ld.data_ptr(), xd.data_ptr(), x0d.data_ptr(), int(call == 0),
                                         call, C.byref(record), torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        assert d['active'].cpu().tolist() == rec['active'], call
        assert d['original'].cpu().tolist() == rec['original'], call
        assert d['adv'].cpu().tolist() == rec['adv'], call
        assert d['found'].cpu().tolist() == rec['found'], call
        got = d['dist'].cpu().tolist()
        for i in range(n):
            if rec['dist'][i] in (0.0, INF):
                assert got[i] == rec['dist'][i], (call, i)
            else:
                rel = abs(got[i] - rec['dist'][i]) / rec['dist'][i]
                print('judge call %d sample %d: distance %.6e, relative error %.1e' % (call, i, got[i], rel))
                assert rel <= 1e-6, (call, i, rel)
            if rec['best'][i] is not None:
                assert torch.equal(d['best'][i].cpu(), rec['best'][i]), (call, i)
            else:
                assert bool((d['best'][i] == -1.0).all()), (call, i)
    # what the scenario was built to contain
    assert rec['original'][3] == 1 and rec['found'][3] == 0 and rec['original'][7] == int(labels[7])
    assert rec['adv'][4] == 0 and rec['found'][5] == -1 and rec['found'][2] == 0
    assert rec['found'][0] == (1 if return_early else 2) and rec['found'][4] == 1 and rec['found'][1] == 2
    assert rec['found'][7] == 2 and rec['found'][6] == 1


def test_attack_entry_points_refuse_bad_arguments():
    from neural_ode_features_amd import _lib
    lib = _lib.load()
    t = torch.zeros(8, device='cuda')
    ok = _lib.NodeAttack(1, 1, 2, 2, 0, 1, 0.1, 0.1, 0.0, 1.0, None, None)
    for bad, word in ((_lib.NodeAttack(1, 1, 2, 2, 1, 1, 0.1, 0.1, 0.0, 1.0, None, None), 'norm'),
                      (_lib.NodeAttack(0, 1, 2, 2, 0, 1, 0.1, 0.1, 0.0, 1.0, None, None), 'shape'),
                      (_lib.NodeAttack(1, 1, 2, 2, 0, 1, 0.1, 0.1, 1.0, 1.0, None, None), 'bounds'),
                      (_lib.NodeAttack(1, 1, 2, 2, 0, 1, 0.1, 0.1, 0.0, 1.0, t.data_ptr(), None), 'mean and std')):
        rc = lib.node_attack_step(C.byref(bad), t.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr(), None)
        assert rc != 0 and word in lib.node_last_error().decode(), (rc, lib.node_last_error())
    assert lib.node_attack_step(C.byref(ok), None, t.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr(), None) == -1

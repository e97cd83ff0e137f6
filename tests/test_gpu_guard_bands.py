"""GPU: every HIP node writes and reads only its own bytes (tests/guarded.py has the allocator, tests/test_guarded_host.py shows
that it catches what it is for).

The parity tests compare a node's outputs with a reference; none of them sees what else the node touched.  PyTorch's caching
allocator rounds blocks up and `workspace.alloc` adds 256 bytes of slack, so a ragged tile written past an output, a write past
the bytes `*_workspace_bytes()` promised or a float4 read past an input goes unnoticed; an output element that is never written
holds the right value of the previous, identical call whose block the allocator hands back; scratch read before it is written
usually holds the same kernel's leftovers.  Here every case -- one node on one small ragged shape, forward and (where the node
has one) backward, through the node's Python entry -- runs

  1. twice with nothing patched: the two result lists (outputs, every gradient, statistics) must be `torch.equal`;
  2. once per fill byte (0xFF: NaN; 0x7F: 3.4e38, what fmaxf, ReLU masks and argmax do not swallow; 0x00) with its workspace
     pools emptied, every input and parameter embedded between bands of the fill, and `workspace.alloc`, `torch.empty`,
     `torch.empty_like` and `torch.zeros` handing out bodies of the fill between bands of at least 1 MiB.  Then, in this order:
     the node RAN (the library's entry points were called, a workspace of exactly the bytes `*_workspace_bytes` returned was
     asked for, the outputs of the expected shapes were created: a `fusable` check that sends the call to ATen fails the test);
     no band byte changed (workspaces with their 256 bytes of slack, outputs, gradients); no input changed, nor its bands; every
     result is `torch.equal` to the plain run's (no tolerance: the same kernels on the same inputs); the loss nodes' zero-contract
     scratch is all zero bits.

Covered: bnfunc, bnhead (+ bn_head_pool_slices), bnstem, bnministem, bnconvstem, bndownconv (+ sliced), bntrunk, bnsolve (forward
and adjoint); the GroupNorm stem and trunk, convstem, ministem, gn_relu_conv, ImageConv2d, max_pool_4s2 / trajectory_pool,
_HeadPool, _GnRelu, linear_cross_entropy, linear + cross_entropy, trajectory_loss, trajectory_distance, the GroupNorm ODE solve
with its adjoint, `odeint`'s backward through the accepted steps and odefunc_vjp; retrieval.average_precision, the SVM fit and cv score, Augmenter, TransferTransform's resize,
the attack step and judge, FusedSGD and FusedAdam.

Left out: graphs.py (a captured graph replays the pointers of its capture: guarded buffers would have to outlive the context; it
needs a test of its own), dp.py (runs across processes), deferred.py (a policy over the solves covered here, no kernel of its
own), generic.py's flat solver (`node_flat_*`: its workspace lives as long as a solve object; tests/test_gpu_generic.py and
tests/test_gpu_step_control.py), the entry points without a Python wrapper that allocates for them (`node_conv3x3_w4`,
`node_stem_conv`, `node_stem_conv0_dgrad`: their tests hand in raw pointers), 16 x 16 states of the
GroupNorm solve (tests/test_gpu_round2.py records that solve as not reproducible run to run).  The attack's two kernels update
buffers that `attack.bim` makes with clone / full, so they run here through the C ABI on embedded buffers.

Not bit-reproducible run to run: none of the nodes at these shapes (NOT_REPRODUCIBLE is empty; a node entered there keeps its
band and input checks and loses the cross-fill equality with an xfail).

Found by these tests: the loss kernels left their workgroup partials in `head`'s zero-contract scratch (only the arrival counters
were reset); csrc/kernels_loss.hip now zeroes each partial as the last workgroup reads it.
"""

import pytest
import torch

from tests import guarded as G

pytestmark = pytest.mark.gpu
DEV = 'cuda'

# node name (the part of a case's name in front of the first space) -> what was seen
NOT_REPRODUCIBLE = {}
CASES = []


def _pools():
    """every workspace pool of the package: the module-level dicts, and the two pools of each of resnet.py's trunk entries"""
    from neural_ode_features_amd import (bnfunc, bnsolve, convstem, downconv, finetune, head, imgconv, integrate, ministem,
                                         resnet, retrieval, stem)
    names = ('_WS', '_FWD', '_BN_FREE', '_BN_SCRATCH', '_SCRATCH', '_FREE', '_LOSS_SCRATCH', '_SLICES_SCRATCH')
    pools = [getattr(m, n) for m in (bnfunc, bnsolve, convstem, downconv, finetune, head, imgconv, integrate, ministem, retrieval, stem)
             for n in names if isinstance(getattr(m, n, None), dict)]
    return pools + [p for e in (resnet._GROUP, resnet._BATCH) for p in (e.free, e.scratch)]


def add(name, build, run, **kw):
    CASES.append(G.Case(name, build, run, **kw))


def _f32(*shapes):
    return [(tuple(s), torch.float32) for s in shapes]


def module_case(name, make, inputs, forward, node=None, calls=(), bytes_fn=None, prepare=None, backward=True, x_grad=True, outputs=None):
    """A node behind an nn.Module: tensors = [x, cotangent, *parameters]; results = [out, d_x, *parameter gradients, *extras].
    forward(mod, x) -> out, or (out, after) with after() -> further result tensors once the backward has run."""
    def build():
        x, cot = inputs()
        return [x, cot] + [p.detach().clone() for p in make().parameters()]

    def run(ts):
        mod = make().to(DEV)
        if prepare:
            prepare(mod)
        params = list(mod.parameters())
        assert len(params) == len(ts) - 2
        for p, t in zip(params, ts[2:]):
            p.data = t
        xg = ts[0].detach().requires_grad_(backward and x_grad)
        with torch.set_grad_enabled(backward):
            out = forward(mod, xg)
        after = None
        if isinstance(out, tuple):
            out, after = out
        if not backward:
            return [out] + (list(after()) if after else [])
        if node:
            assert type(out.grad_fn).__name__ == node, (name, type(out.grad_fn).__name__)          # the node, not the module sequence
        out.backward(ts[1])
        return [out.detach()] + ([xg.grad] if x_grad else []) + [p.grad for p in params] + (list(after()) if after else [])

    def default_outputs():          # the output, the input's gradient, every parameter's
        ts = build()
        return _f32(*([ts[1].shape] + ([t.shape for t in ([ts[0]] if x_grad else []) + ts[2:]] if backward else [])))
    add(name, build, run, calls=calls, bytes_fn=bytes_fn, outputs=outputs or default_outputs)


# ---------------------------------------------------------------------------------------------------------------------------------
# batch-norm nodes
# ---------------------------------------------------------------------------------------------------------------------------------
def _bn_cases():
    from tests import bnconvstem_cases as KC
    from tests import bnfunc_cases as B
    from tests import bnhead_cases as H
    from tests import bnministem_cases as KM
    from tests import bnsolve_cases as SV
    from tests import bnstem_cases as S
    from tests import bntrunk_cases as T
    from tests import trajhead_cases as TH

    for case in [(3, 64, 7, 7), (1, 64, 6, 5)]:
        seed = B.SEEDS[case]

        def forward(mod, x):
            tg = torch.tensor(B.T_EVAL, dtype=torch.float32, device=DEV).requires_grad_(True)
            return mod(tg, x), lambda: [tg.grad]
        module_case('bnfunc %s' % (case,), lambda case=case, seed=seed: B.func_pair(case[1], seed)[0],
                    lambda case=case, seed=seed: B.case_inputs(case, seed), forward, '_BatchOdeFnBackward',
                    ['node_bnfunc_fwd', 'node_bnfunc_bwd'], 'node_bnfunc_workspace_bytes')

        # the classifier head behind the same shapes, with and without a dropout scale
        for dropout in (False, True):
            hseed = H.SEEDS[case]

            def build(case=case, hseed=hseed, dropout=dropout):
                z, cot, scale = H.case_inputs(case, hseed)
                bn = H.norm_pair(case, hseed)[0]
                return [z, cot, bn.weight.detach().clone(), bn.bias.detach().clone()] + ([scale] if dropout else [])

            def run(ts, dropout=dropout):
                from neural_ode_features_amd import head
                z, g, b = (t.detach().requires_grad_(True) for t in (ts[0], ts[2], ts[3]))
                pooled = head._BnHeadPool.apply(z, g, b, ts[4] if dropout else None, 1e-5)
                pooled.backward(ts[1])
                return [pooled.detach(), z.grad, g.grad, b.grad]
            n, c = case[:2]
            add('bnhead %s%s' % (case, ' scale' if dropout else ''), build, run, calls=['node_bnhead_fwd', 'node_bnhead_bwd'],
                outputs=_f32((n, c), (2, c), case))

    tcase = TH.CPU_HEAD_CASES[0]          # (3, 2, 64, 5, 5): 50 rows per slice, a ragged 32-row trip

    def build_slices():
        bn = H.norm_pair(tcase[1:], TH.seed_of(tcase))[0]
        return [TH.trajectory(tcase), bn.weight.detach().clone(), bn.bias.detach().clone()]

    def run_slices(ts):
        from neural_ode_features_amd import head
        with torch.no_grad():
            return [head.bn_head_pool_slices(ts[0], ts[1], ts[2], 1e-5)]
    add('bn_head_pool_slices %s' % (tcase,), build_slices, run_slices, calls=['node_bnhead_fwd_slices'],
        outputs=_f32(tcase[:3], (tcase[0], 2, tcase[2])))

    def input_grad(mod):
        mod.input_grad = True

    def fused_input_grad(mod):
        mod.fused_batch = True
        mod.input_grad = True

    for case in [(1, 28, 64, 2), (1, (6, 5), 64, 4)]:
        module_case('bnstem %s' % (case,), lambda case=case: S.stem_pair(case, S.SEEDS[case])[0], lambda case=case: S.case_inputs(case, S.SEEDS[case]),
                    lambda m, x: m(x), '_BnStemFnBackward', ['node_bnstem_fwd', 'node_bnstem_bwd'], 'node_bnstem_workspace_bytes', input_grad)
    for case in [(1, 10, 64, 1), (3, (12, 10), 64, 2)]:
        module_case('bnministem %s' % (case,), lambda case=case: KM.module_pair(case, KM.SEEDS[case])[0],
                    lambda case=case: KM.case_inputs(case, KM.SEEDS[case]), lambda m, x: m(x), '_BnMiniStemFnBackward',
                    ['node_bnministem_fwd', 'node_bnministem_bwd'], 'node_bnministem_workspace_bytes', fused_input_grad)
    ccase = ('stem', 1, 28, 64, 2)
    module_case('bnconvstem %s' % (ccase,), lambda: KC.module_pair(ccase, KC.SEEDS[ccase])[0], lambda: KC.case_inputs(ccase, KC.SEEDS[ccase]),
                lambda m, x: m(x), '_BnConvStemFnBackward', ['node_bnconvstem_fwd', 'node_bnconvstem_bwd_dx'], 'node_bnconvstem_workspace_bytes',
                input_grad)

    def down(mod, x, slices=1):
        from neural_ode_features_amd import downconv
        return downconv.bn_relu_conv(x, mod[0], mod[2], slices)
    dcase = ('down', 2, 64, 64, 4)
    module_case('bndownconv %s' % (dcase,), lambda: KC.module_pair(dcase, KC.seed_of(dcase, 'kinkfree'), 'kinkfree')[0],
                lambda: KC.case_inputs(dcase, KC.seed_of(dcase, 'kinkfree')), down, '_BnDownConvFnBackward',
                ['node_bndownconv_fwd', 'node_bndownconv_bwd'], 'node_bndownconv_workspace_bytes')
    scase = ('sliced', 3, 2, 64, (7, 6))          # forward only: the library refuses slices > 1 with a backward to come

    def sliced_inputs():
        x, cot = KC.case_inputs(scase, KC.seed_of(scase, 'kinkfree'))
        return x.reshape(-1, *x.shape[2:]), cot.reshape(-1, *cot.shape[2:])
    module_case('bndownconv %s' % (scase,), lambda: KC.module_pair(scase, KC.seed_of(scase, 'kinkfree'), 'kinkfree')[0], sliced_inputs,
                lambda m, x: down(m, x, scase[1]), None, ['node_bndownconv_fwd'], 'node_bndownconv_workspace_bytes', backward=False)

    tcase2 = (64, 7, 3, 2)

    def taps_forward(mod, x):
        out, taps = mod.forward_taps(x)
        return out, lambda: list(taps)
    module_case('bntrunk %s' % (tcase2,), lambda: T.trunk_pair(tcase2, T.SEEDS[tcase2])[0], lambda: T.case_inputs(tcase2, T.SEEDS[tcase2]),
                taps_forward, '_BnTrunkFnBackward', ['node_bntrunk_fwd', 'node_bntrunk_bwd'], 'node_bntrunk_workspace_bytes')

    shape, grid = (4, 64, 6, 6), (0.0, 0.3, 0.55, 1.0)

    def solve_forward(mod, x):
        import neural_ode_features_amd as nof
        return nof.odeint_adjoint(mod, x, torch.tensor(grid, dtype=torch.float32).to(DEV), rtol=1e-3, atol=1e-3, method='dopri5')
    module_case('bnsolve %s' % (shape,), lambda: B.func_pair(shape[1], SV.SEED, True)[0], lambda: SV.inputs(shape, grid), solve_forward, None,
                ['node_bnsolve_fwd', 'node_bnsolve_adjoint'], 'node_bnsolve_workspace_bytes',
                lambda m: setattr(m, 'batch_solve', True))          # (off by default: without it the generic solver runs, and this case fails)


# ---------------------------------------------------------------------------------------------------------------------------------
# GroupNorm nodes
# ---------------------------------------------------------------------------------------------------------------------------------
def _gn_head_cases():
    def gn_params(c, gen):
        return 1.0 + 0.25 * torch.randn(c, generator=gen), 0.1 * torch.randn(c, generator=gen)

    for shape in [(5, 64, 7, 7), (2, 8, 5, 6), (7, 16, 2, 2)]:
        for with_scale in (False, True):
            def build(shape=shape, with_scale=with_scale):
                gen = torch.Generator().manual_seed(11 + sum(shape))
                n, c = shape[:2]
                g, b = gn_params(c, gen)
                ts = [torch.randn(*shape, generator=gen), torch.randn(n, c, generator=gen), g, b]
                return ts + ([(torch.rand(n, c, generator=gen) < 0.5).float() * 2.0] if with_scale else [])

            def run(ts, shape=shape, with_scale=with_scale):
                from neural_ode_features_amd import head
                z, g, b = (t.detach().requires_grad_(True) for t in (ts[0], ts[2], ts[3]))
                pooled = head._HeadPool.apply(z, g, b, ts[4] if with_scale else None, min(32, shape[1]), 1e-5)
                pooled.backward(ts[1])
                return [pooled.detach(), z.grad, g.grad, b.grad]
            n, c = shape[:2]
            groups = min(32, c)
            add('head_pool %s%s' % (shape, ' scale' if with_scale else ''), build, run, calls=['node_head_fwd', 'node_head_bwd'],
                outputs=_f32((n, c), (n, groups, 2), shape, (n + 1, 2, c)))

    for shape in [(3, 96, 5, 7), (2, 8, 3, 3)]:
        for relu in (True, False):
            def build(shape=shape):
                gen = torch.Generator().manual_seed(12 + sum(shape))
                g, b = gn_params(shape[1], gen)
                return [torch.randn(*shape, generator=gen), torch.randn(*shape, generator=gen), g, b]

            def run(ts, shape=shape, relu=relu):
                from neural_ode_features_amd import head
                norm = torch.nn.GroupNorm(min(32, shape[1]), shape[1]).to(DEV)
                norm.weight.data, norm.bias.data = ts[2], ts[3]
                z = ts[0].detach().requires_grad_(True)
                out = head.gn_relu(z, norm, relu)
                assert type(out.grad_fn).__name__ == '_GnReluBackward'
                out.backward(ts[1])
                return [out.detach(), z.grad, norm.weight.grad, norm.bias.grad]
            n, c = shape[:2]
            add('gn_relu %s relu=%d' % (shape, relu), build, run, calls=['node_gn_relu_fwd', 'node_gn_relu_bwd'],
                outputs=_f32(shape, (n, min(32, c), 2), (n + 1, 2, c)))

    def loss_scratch():
        from neural_ode_features_amd import head
        return list(head._LOSS_SCRATCH.values()) + list(head._SLICES_SCRATCH.values())

    for n, c, o in [(7, 64, 10), (5, 20, 3), (130, 64, 33)]:
        def build(n=n, c=c, o=o):
            gen = torch.Generator().manual_seed(13 + n + c + o)
            return [torch.rand(n, c, generator=gen), torch.randn(o, c, generator=gen) / c ** 0.5, 0.1 * torch.randn(o, generator=gen),
                    torch.randint(0, o, (n,), generator=gen)]

        def run_fused(ts):
            from neural_ode_features_amd import head
            p, w, b = (t.detach().requires_grad_(True) for t in ts[:3])
            loss, logits = head.linear_cross_entropy(p, w, b, ts[3])
            assert type(loss.grad_fn).__name__ == '_LinearCrossEntropyBackward'
            loss.backward()
            return [loss.detach(), logits.detach(), loss.node_stat, p.grad, w.grad, b.grad]

        def run_pair(ts):
            from neural_ode_features_amd import head
            p, w, b = (t.detach().requires_grad_(True) for t in ts[:3])
            logits = head.linear(p, w, b)
            assert type(logits.grad_fn).__name__ == '_LinearBackward'
            loss = head.cross_entropy(logits, ts[3], reduction='sum')
            assert type(loss.grad_fn).__name__ == '_LinearCrossEntropyBackward'
            loss.backward()
            return [loss.detach(), logits.detach(), loss.node_stat, p.grad, w.grad, b.grad]

        def run_loss_alone(ts):
            from neural_ode_features_amd import head
            p, w, b = (t.detach().requires_grad_(True) for t in ts[:3])
            logits = head.linear(p, w, b)
            logits = logits * 1.0                       # no longer `linear`'s own result: the plain edges, _CrossEntropy then _Linear
            loss = head.cross_entropy(logits, ts[3])
            assert type(loss.grad_fn).__name__ == '_CrossEntropyBackward'
            loss.backward()
            return [loss.detach(), logits.detach(), loss.node_stat, p.grad, w.grad, b.grad]
        outs = _f32((), (2,), (n, o), (n, c), (o, c), (o,))
        add('linear_cross_entropy %s' % ((n, c, o),), build, run_fused, calls=['node_head_loss_fwd', 'node_head_loss_bwd'], outputs=outs,
            zero_scratch=loss_scratch)
        add('linear+cross_entropy %s' % ((n, c, o),), build, run_pair, calls=['node_head_loss_fwd', 'node_head_loss_bwd'], outputs=outs,
            zero_scratch=loss_scratch)
        add('linear,cross_entropy %s' % ((n, c, o),), build, run_loss_alone, calls=['node_head_loss_fwd', 'node_head_loss_bwd'], outputs=outs,
            zero_scratch=loss_scratch)

    from tests import trajhead_cases as TH
    lcase = (21, 7, 64, 10)          # T = 21 slices of 7 samples: nothing a multiple of anything

    def build_tl():
        pooled, weight, bias, target = TH.loss_inputs(lcase)
        return [torch.einsum('tnc,oc->tno', pooled, weight) + bias, target]

    def run_tl(ts):
        from neural_ode_features_amd import head
        return [head.trajectory_loss(ts[0], ts[1])]
    add('trajectory_loss %s' % (lcase,), build_tl, run_tl, calls=['node_head_loss_slices_fwd'], outputs=_f32((lcase[0], 2)), zero_scratch=loss_scratch)

    dcase = (2, 3, 64, 7, 7)         # H W % 4 != 0: the one-thread-per-channel kernel

    def build_td():
        traj0, traj1, norm = TH.distance_case(dcase)[:3]
        return [traj0, traj1, norm.weight.detach().clone(), norm.bias.detach().clone()]

    def run_td(ts):
        from neural_ode_features_amd import head
        norm = torch.nn.GroupNorm(32, dcase[2]).to(DEV)
        norm.weight.data, norm.bias.data = ts[2], ts[3]
        l2, cos = head.trajectory_distance(ts[0], ts[1], norm)
        return [l2, cos]
    add('trajectory_distance %s' % (dcase,), build_td, run_td, calls=['node_gn_relu_distance'], outputs=_f32(dcase[:2] + (2,)))


def _gn_stem_cases():
    from tests import stem_geometry_cases as SG
    for name in ('r7x12_f128', 's5_f256', 't512_5x6'):
        assert name in SG.CASES and name + '/w4off' not in SG.CASES          # (neither stem row takes the F(4x4,3x3) pipeline: no twin)
        kind = SG.row_of(name)[0]

        def make(name=name):
            return SG.modules(name)[1]

        def inputs(name=name):
            return SG.modules(name)[3:]
        if kind == 'stem':
            module_case('stem ' + name, make, inputs, lambda m, x: m(x), '_StemFnBackward', ['node_stem_fwd', 'node_stem_bwd'],
                        'node_stem_workspace_bytes', x_grad=False)
            module_case('stem ' + name + ' input_grad', make, inputs, lambda m, x: m(x), '_StemFnBackward', ['node_stem_fwd', 'node_stem_bwd_dx'],
                        'node_stem_workspace_bytes', lambda m: setattr(m, 'input_grad', True))
        else:
            module_case('trunk ' + name, make, inputs, lambda m, x: m(x), None, ['node_trunk_fwd', 'node_trunk_bwd'], 'node_trunk_workspace_bytes')


def _gn_solve_cases():
    from tests.helpers import make_func
    for shape in [(3, 64, 7, 7), (6, 64, 8, 8)]:
        def inputs(shape=shape):
            gen = torch.Generator().manual_seed(142)
            return torch.randn(*shape, generator=gen), torch.randn(3, *shape, generator=gen)

        def solve(mod, x):
            import neural_ode_features_amd as nof
            return nof.odeint_adjoint(mod, x, torch.tensor([0.0, 0.3, 1.0]).to(DEV), rtol=1e-4, atol=1e-4, method='dopri5')
        module_case('solve %s' % (shape,), lambda shape=shape: make_func(shape[1], seed=141)[0], inputs, solve, None,
                    ['node_solve_fwd', 'node_solve_adjoint'], 'node_workspace_bytes', outputs=_f32((3,) + shape, shape))

        def backprop(mod, x):
            import neural_ode_features_amd as nof
            return nof.odeint(mod, x, torch.tensor([0.0, 0.3, 1.0]).to(DEV), rtol=1e-4, atol=1e-4, method='dopri5')
        if shape == (3, 64, 7, 7):
            module_case('odeint %s' % (shape,), lambda shape=shape: make_func(shape[1], seed=141)[0], inputs, backprop, None,
                        ['node_solve_fwd', 'node_solve_backprop'], 'node_backprop_workspace_bytes', outputs=_f32((3,) + shape, shape))

        def build_vjp(shape=shape, inputs=inputs):
            x, cot = inputs()
            return [x, cot[0].clone()] + [p.detach().clone() for p in make_func(shape[1], seed=141)[0].parameters()]

        def run_vjp(ts, shape=shape):
            import neural_ode_features_amd as nof
            f = make_func(shape[1], seed=141)[0].to(DEV)
            for p, t in zip(f.parameters(), ts[2:]):
                p.data = t
            fo, vy, vt, vp = nof.odefunc_vjp(f, 0.2, ts[0], ts[1])
            return [fo, vy, vt, vp, nof.odefunc_forward(f, 0.2, ts[0])]
        add('odefunc_vjp %s' % (shape,), build_vjp, run_vjp, calls=['node_odefunc_vjp', 'node_odefunc_fwd'], bytes_fn='node_workspace_bytes',
            outputs=_f32(shape, (1,)))


def _gn_conv_cases():
    def stem_pair(kind, in_ch, filters, kink_free):          # tests/test_gpu_convstem.py::_stem_pair, tests/test_gpu_ministem.py::_pair
        import neural_ode_features_amd as nof
        seed = in_ch + filters
        torch.manual_seed(seed)
        stem = nof.ODENet(in_ch, out=10, n_filters=filters, downsample=kind, adjoint=True).downsample.module
        gen = torch.Generator().manual_seed(seed + 1)
        with torch.no_grad():
            for i in (1, 4):
                for p in (stem[i].weight, stem[i].bias):
                    p.add_(0.2 * torch.randn(p.shape, generator=gen))
                if kink_free:
                    stem[i].bias.add_(8.0)
        return stem

    def stem_inputs(make, n, in_ch, h, w):
        gen = torch.Generator().manual_seed(99)
        x = torch.randn(n, in_ch, h, w, generator=gen)
        with torch.no_grad():
            shape = make()(x).shape
        return x, torch.randn(shape, generator=gen)

    def input_grad(mod):
        mod.input_grad = True
    # test_gpu_convstem.py's cases are 32 x 32 (30 -> 15 -> 7) and 28 x 28 (26 -> 13 -> 6): the second is the smaller and the more ragged
    make_c = lambda: stem_pair('convolution', 1, 64, True)
    module_case('convstem in1_28x28_f64_n5', make_c, lambda: stem_inputs(make_c, 5, 1, 28, 28), lambda m, x: m(x), '_ConvStemFnBackward',
                ['node_convstem_fwd', 'node_convstem_bwd'], 'node_convstem_workspace_bytes', x_grad=False)
    module_case('convstem in1_28x28_f64_n5 input_grad', make_c, lambda: stem_inputs(make_c, 5, 1, 28, 28), lambda m, x: m(x), '_ConvStemFnBackward',
                ['node_convstem_fwd', 'node_convstem_bwd_dx'], 'node_convstem_workspace_bytes', input_grad)
    # test_gpu_ministem.py: (3, 14, 22, 64, 3) is its one rectangular case, 12 x 20 -> 6 x 10 -> 3 x 5, odd batch
    make_m = lambda: stem_pair('minimal', 3, 64, False)
    module_case('ministem in3_14x22_f64_n3', make_m, lambda: stem_inputs(make_m, 3, 3, 14, 22), lambda m, x: m(x), '_MiniStemFnBackward',
                ['node_ministem_fwd', 'node_ministem_bwd'], 'node_ministem_workspace_bytes', input_grad)

    # test_gpu_downconv.py: (2, 64, 256, 15, 15) has the odd sides (15 -> 7: the last input row and column are read by no window),
    # (5, 128, 128, 8, 6) the rectangle and the odd batch
    for n, cin, cout, h, w in [(2, 64, 256, 15, 15), (5, 128, 128, 8, 6)]:
        def make(cin=cin, cout=cout, h=h):
            seed = cin + cout + h
            torch.manual_seed(seed)
            mod = torch.nn.Sequential(torch.nn.GroupNorm(min(32, cin), cin), torch.nn.ReLU(), torch.nn.Conv2d(cin, cout, 4, 2, 1))
            gen = torch.Generator().manual_seed(seed + 1)
            with torch.no_grad():
                for p in (mod[0].weight, mod[0].bias):
                    p.add_(0.2 * torch.randn(p.shape, generator=gen))
            return mod

        def inputs(n=n, cin=cin, cout=cout, h=h, w=w):
            gen = torch.Generator().manual_seed(99 + n)
            return torch.randn(n, cin, h, w, generator=gen), torch.randn(n, cout, (h - 2) // 2 + 1, (w - 2) // 2 + 1, generator=gen)

        def forward(mod, x):
            from neural_ode_features_amd.downconv import gn_relu_conv
            return gn_relu_conv(x, mod[0], mod[2])
        module_case('gn_relu_conv n%d_c%d-%d_%dx%d' % (n, cin, cout, h, w), make, inputs, forward, '_DownConvFnBackward',
                    ['node_downconv_fwd', 'node_downconv_bwd'], 'node_downconv_workspace_bytes')

    # test_gpu_imgconv.py: (5, 3, 8, 8, 64) is the smallest with an odd batch, (37, 3, 12, 20, 128) the rectangle whose batch no tile divides
    for n, cin, h, w, filters in [(5, 3, 8, 8, 64), (37, 3, 12, 20, 128)]:
        for bias in (True, False):
            def make(cin=cin, filters=filters, bias=bias):
                import neural_ode_features_amd as nof
                torch.manual_seed(7)
                return nof.ImageConv2d(cin, filters, bias=bias)

            def inputs(n=n, cin=cin, h=h, w=w, filters=filters):
                gen = torch.Generator().manual_seed(8)
                return torch.randn(n, cin, h, w, generator=gen), torch.randn(n, filters, h // 2, w // 2, generator=gen)

            def forward(mod, x):
                out = mod(x)
                assert type(out.grad_fn).__name__.startswith('_ImgConvFn')
                return out
            module_case('imgconv %s%s' % ((n, cin, h, w, filters), '' if bias else ' no bias'), make, inputs, forward, None,
                        ['node_imgconv_fwd', 'node_imgconv_bwd'], 'node_imgconv_workspace_bytes')

    # test_gpu_pool.py: (1, 3, 5, 9) odd and rectangular, (2, 65, 7, 7) an odd channel count, (2, 8, 2, 2) the floor (one window)
    for shape in [(1, 3, 5, 9), (2, 65, 7, 7), (2, 8, 2, 2)]:
        for kind in ('randn', 'ties'):
            def build(shape=shape, kind=kind):
                gen = torch.Generator().manual_seed(sum(shape))
                x = torch.randint(0, 3, shape, generator=gen).float() if kind == 'ties' else torch.randn(shape, generator=gen)
                oh, ow = (shape[2] - 2) // 2 + 1, (shape[3] - 2) // 2 + 1
                return [x, torch.randn(shape[0], shape[1], oh, ow, generator=gen)]

            def run(ts):
                from neural_ode_features_amd import pool
                x = ts[0].detach().requires_grad_(True)
                y = pool.max_pool_4s2(x)
                assert type(y.grad_fn).__name__ == '_MaxPool4s2FnBackward'
                y.backward(ts[1])
                return [y.detach(), x.grad]
            oh, ow = (shape[2] - 2) // 2 + 1, (shape[3] - 2) // 2 + 1
            add('max_pool_4s2 %s %s' % (shape, kind), build, run, calls=['node_pool_fwd', 'node_pool_bwd'],
                outputs=_f32(shape[:2] + (oh, ow), shape) + [(shape[:2] + (oh, ow), torch.uint8)])
    tshape = (4, 2, 65, 7, 7)

    def build_tp():
        return [torch.randn(tshape, generator=torch.Generator().manual_seed(21))]

    def run_tp(ts):
        from neural_ode_features_amd import pool
        with torch.no_grad():
            means, pooled = pool.trajectory_pool(ts[0])
        return [means, pooled]
    add('trajectory_pool %s' % (tshape,), build_tp, run_tp, calls=['node_pool_fwd'], outputs=_f32(tshape[:3], tshape[1:3] + (3, 3)))


# ---------------------------------------------------------------------------------------------------------------------------------
# evaluation and optimiser nodes
# ---------------------------------------------------------------------------------------------------------------------------------
def _eval_cases():
    for nq, nd, d in [(5, 7, 20), (33, 1000, 64)]:
        def build(nq=nq, nd=nd, d=d):
            gen = torch.Generator().manual_seed(31 + nq)          # integer features: every score is exact, ties included
            return [torch.randint(-3, 4, (nq, d), generator=gen).float(), torch.randint(-3, 4, (nd, d), generator=gen).float(),
                    torch.randint(0, 4, (nq,), generator=gen, dtype=torch.int32), torch.randint(0, 4, (nd,), generator=gen, dtype=torch.int32)]

        def run(ts):
            from neural_ode_features_amd import retrieval
            ap, ap_k = retrieval.average_precision(ts[0], ts[1], ts[2], ts[3], k=3)
            return [ap, ap_k]
        add('retrieval nq%d_nd%d_d%d' % (nq, nd, d), build, run, calls=['node_retrieval_ap'], bytes_fn='node_retrieval_workspace_bytes',
            outputs=[((nq,), torch.float64)])

    from tests import svm_reference as R
    scase = R.CASES[0]          # (37, 1, 63, 11): one ragged slab of rows, D + 1 = 2, one problem short of a tile

    def build_svm():
        cd = R.case_data(scase)
        return [torch.from_numpy(cd.x).float(), torch.from_numpy(cd.labels).to(torch.int32), torch.from_numpy(cd.row_fold).to(torch.int32)]

    def run_svm(ts):
        import numpy as np
        from neural_ode_features_amd import finetune
        cd = R.case_data(scase)
        table = finetune.problem_table(cd.folds, cd.classes, cd.cs)
        w, info = finetune.linear_svc_fit(ts[0], ts[1], ts[2], table)
        correct, held, pred = finetune.svc_cv_score(ts[0], ts[1], ts[2], table, w, np.arange(len(table)).reshape(-1, 1), neg_class=77, return_pred=True)
        return [w, torch.from_numpy(np.ascontiguousarray(info['iterations']).astype(np.int64)), torch.from_numpy(info['grad_ratio'].astype(np.float64)),
                torch.from_numpy(correct.astype(np.int64)), torch.from_numpy(held.astype(np.int64)), torch.from_numpy(pred.astype(np.int64))]
    n, d, p, _ = scase
    add('svm %s' % (scase,), build_svm, run_svm, calls=['node_svm_fit', 'node_svm_cv_score'], bytes_fn='node_svm_workspace_bytes',
        outputs=[((p, d + 1), torch.float32), ((2, p), torch.int32), ((p, n), torch.int32)])

    def images(c, h, w, seed):
        gen = torch.Generator().manual_seed(seed)
        return [torch.randint(0, 256, (9, c, h, w), generator=gen, dtype=torch.uint8), torch.randint(0, 10, (9,), generator=gen),
                torch.tensor([8, 0, 3, 3, 5])]          # a batch of 5 of the 9 images, one of them twice, the last image among them

    for kind, c, side in [('crop+jitter+flip+norm', 3, 32), ('crop', 1, 28)]:
        def run(ts, kind=kind, c=c):
            from neural_ode_features_amd import augment
            split = augment.DeviceSplit(ts[0], ts[1], DEV)
            assert split.x.data_ptr() == ts[0].data_ptr() and split.y.data_ptr() == ts[1].data_ptr()
            aug = augment.Augmenter(kind, dataset='cifar10' if c == 3 else 'mnist', seed=5)
            out = list(aug.batch(split, ts[2], epoch=3))
            return out + list(aug.batch(split, ts[2], epoch=0, train=False))
        add('augment %s %dx%dx%d' % (kind, c, side, side), lambda c=c, side=side: images(c, side, side, 41), run, calls=['node_augment_batch'],
            outputs=[((5, c, side, side), torch.float32), ((5,), torch.int64)])

    for c, h, w, size in [(3, 7, 9, (12, 5)), (1, 28, 28, 32)]:          # up in one direction and down in the other; the reference's MNIST -> 32
        def run(ts, c=c, size=size):
            from neural_ode_features_amd import augment
            split = augment.DeviceSplit(ts[0], ts[1], DEV)
            tt = augment.TransferTransform(size, dataset='cifar10' if c == 3 else 'mnist')
            img, target = tt.batch(split, ts[2])
            return [img, target, tt.resized(split, ts[2])]
        hw = size if isinstance(size, tuple) else (size, size)
        add('resize %dx%dx%d to %s' % (c, h, w, hw), lambda c=c, h=h, w=w: images(c, h, w, 43), run, calls=['node_resize_batch'],
            outputs=[((5, c) + hw, torch.float32), ((5, c) + hw, torch.uint8), ((5,), torch.int64)])

    # the attack's two kernels work in place on buffers that `bim` makes with clone / full: here through the C ABI, as
    # tests/test_gpu_attack_kernels.py calls them, on its smallest shape (105 elements per sample: tails in every reduction)
    import ctypes as C
    ashape = (2, 3, 5, 7)
    for norm in (float('inf'), 2):
        def build(norm=norm):
            from tests.test_gpu_attack_kernels import _inputs
            x0, x, g, active, _ = _inputs(ashape, 0, 17)
            gen = torch.Generator().manual_seed(18)
            n = ashape[0]
            return [x0, g, torch.randint(0, 10, (n,), generator=gen), torch.randn(n, 10, generator=gen),           # inputs
                    torch.tensor([0.4914, 0.4822, 0.4465]), torch.tensor([0.2023, 0.1994, 0.2010]),
                    x, torch.full(ashape, 7.0), active,                                                                 # updated in place: x, xn, the record
                    torch.full((n,), -1, dtype=torch.int32), torch.full((n,), -1, dtype=torch.int32), torch.full((n,), -1, dtype=torch.int32),
                    torch.full((n,), float('inf')), torch.zeros(ashape)]

        def run(ts, norm=norm):
            from neural_ode_features_amd import _lib
            lib = _lib.load()
            x0, g, labels, logits, mean, std, x, xn, active, original, adv_class, found, distance, best = ts
            n, c, h, w = ashape
            atk = _lib.NodeAttack(n, c, h, w, _lib.ATTACK_LINF if norm == float('inf') else _lib.ATTACK_L2, 0, 0.01, 0.03, 0.0, 1.0,
                                  mean.data_ptr(), std.data_ptr())
            rec = _lib.NodeAttackRecord(active.data_ptr(), original.data_ptr(), adv_class.data_ptr(), found.data_ptr(), distance.data_ptr(),
                                        best.data_ptr())
            stream = torch.cuda.current_stream().cuda_stream
            _lib.check(lib.node_attack_judge(C.byref(atk), logits.shape[1], logits.data_ptr(), labels.data_ptr(), x.data_ptr(), x0.data_ptr(),
                                             1, 0, C.byref(rec), stream))
            _lib.check(lib.node_attack_step(C.byref(atk), x.data_ptr(), x0.data_ptr(), g.data_ptr(), active.data_ptr(), xn.data_ptr(), stream))
            _lib.check(lib.node_attack_judge(C.byref(atk), logits.shape[1], logits.data_ptr(), labels.data_ptr(), x.data_ptr(), x0.data_ptr(),
                                             0, 1, C.byref(rec), stream))
            return [x, xn, active, original, adv_class, found, distance, best]
        add('attack %s norm=%s' % (ashape, norm), build, run, calls=['node_attack_judge', 'node_attack_step'], writes=range(6, 14))

    # FusedSGD / FusedAdam: nothing is allocated in a step (the state is handed in), so the bands, the gradients and the equality of the
    # updated tensors are what applies.  Sizes 1, 257, 8 x 16 and 1023; gradients once aligned, once at odd float offsets of one buffer.
    sizes = [(1,), (257,), (8, 16), (1023,)]
    numel = [1, 257, 128, 1023]
    for opt_name, n_state in (('FusedSGD', 1), ('FusedAdam', 2)):
        for odd in (False, True):
            for skip in (False, True):
                def build(n_state=n_state, odd=odd, skip=skip):
                    gen = torch.Generator().manual_seed(51)
                    params = [torch.randn(s, generator=gen) for s in sizes]
                    if odd:
                        grads = [torch.randn(sum(numel) + len(numel) + 1, generator=gen)]          # one buffer, every gradient one float further off
                    else:
                        grads = [torch.randn(s, generator=gen) for s in sizes]
                    state = [0.1 * torch.rand(s, generator=gen) for s in sizes for _ in range(n_state)]
                    steps = [torch.full((), 3.0) for _ in sizes] if n_state == 2 else []
                    return params + state + steps + [torch.tensor([1.0 if skip else 0.0])] + grads

                def run(ts, opt_name=opt_name, n_state=n_state, odd=odd):
                    import neural_ode_features_amd as nof
                    k = len(sizes)
                    params = [torch.nn.Parameter(t, requires_grad=True) for t in ts[:k]]
                    state = ts[k:k + k * n_state]
                    steps = ts[k + k * n_state:k + k * n_state + (k if n_state == 2 else 0)]
                    flag = ts[k + k * n_state + len(steps)]
                    grads = ts[k + k * n_state + len(steps) + 1:]
                    assert all(p.data_ptr() == t.data_ptr() for p, t in zip(params, ts))
                    if opt_name == 'FusedSGD':
                        opt = nof.FusedSGD(params, lr=0.1, momentum=0.9, weight_decay=1e-4)
                        for i, p in enumerate(params):
                            opt.state[p]['momentum_buffer'] = state[i]
                    else:
                        opt = nof.FusedAdam(params, lr=1e-2, weight_decay=1e-4)
                        for i, p in enumerate(params):
                            opt.state[p].update(step=steps[i], exp_avg=state[2 * i], exp_avg_sq=state[2 * i + 1])
                    opt.skip_flag = flag
                    off = 1
                    for i, p in enumerate(params):
                        if odd:
                            p.grad = grads[0][off:off + p.numel()].view(p.shape)
                            assert p.grad.data_ptr() % 16 != 0
                            off += p.numel() + 1
                        else:
                            p.grad = grads[i]
                    opt.step()
                    return [p.detach() for p in params] + list(state) + list(steps)
                n_updated = len(sizes) * (1 + n_state) + (len(sizes) if n_state == 2 else 0)
                add('%s%s%s' % (opt_name, ' odd offsets' if odd else '', ' skip' if skip else ''), build, run,
                    calls=['node_sgd_step' if opt_name == 'FusedSGD' else 'node_adam_step'], writes=() if skip else range(n_updated))


_bn_cases()
_gn_head_cases()
_gn_stem_cases()
_gn_conv_cases()
_gn_solve_cases()
_eval_cases()
POOLS = None


@pytest.mark.parametrize('case', CASES, ids=repr)
def test_node_touches_only_its_own_bytes(case):
    global POOLS
    if POOLS is None:
        POOLS = _pools()
    case.pools = POOLS
    node = case.name.split(' ')[0]
    compare = node not in NOT_REPRODUCIBLE
    if compare:
        plain = G.plain_run(case, DEV)
    else:
        tensors = case.build()
        plain = [r.detach().cpu() for r in case.run([t.to(DEV) for t in tensors])]
    try:
        for fill in G.FILLS:
            G.guarded_run(case, fill, plain, DEV, compare)
    except RuntimeError as e:
        if 'HIP error' in str(e) or 'illegal memory access' in str(e):          # the device context is gone: nothing after this can run
            pytest.exit('GPU fault in %s: %s' % (case.name, e), returncode=3)
        raise
    if not compare:
        pytest.xfail('%s is not bit-reproducible run to run (%s): bands and inputs hold, the cross-fill equality is not asserted'
                     % (node, NOT_REPRODUCIBLE[node]))

"""Cases, inputs, references and error measures shared by tests/test_gpu_bnsolve.py and tests/test_bnsolve_host.py: whole solves of
the `norm='batch'` dynamics inside the library (bnsolve.py, csrc/bnsolve_api.hip).

The reference of every comparison is `oracle.torchdiffeq_restated.odeint_adjoint` on the CPU copy of the function (fp64 for the
rk4 runs, fp32 for the dopri5 runs), never the code under test.  Parameters come from tests/bnfunc_cases.py (`func_pair`, seed 5,
ordinary and kink-free); the state is seeded 4, the weights of the loss 7 and scaled by numel ** -0.5, as in
tests/test_gpu_bnfunc.py.

Run through the oracle on the CPU in fp32 and fp64, every shape x grid below takes the same dopri5 steps in both precisions, and
fp32 differs from fp64 by at most 1.3e-6 (outputs), 1.9e-6 (grad_y0) and 1.2e-3 (parameter gradients, by `param_errors`), for rk4
and dopri5 alike: E_FLOOR is those figures rounded up."""
import copy
import functools

import torch

from tests import bnfunc_cases as B

SEED = B.KINK_FREE_SEED      # 5
# (N, C, H, W)
SHAPES = [(4, 64, 6, 6),     # 144 rows: five statistic chunks, the last one partial
          (2, 64, 6, 5),     # non-square
          (1, 64, 3, 3),     # one sample, the smallest image, one chunk
          (2, 192, 7, 7)]    # three column tiles, not a power of two
SPLITK_SHAPE = (64, 64, 8, 8)      # 4096 rows in 128 statistic chunks of 32 rows (one trip of the passes' row loops, like every shape above); a
#                                    weight gradient split 64 ways
MULTIROW_SHAPE = (84, 64, 7, 7)    # 4116 rows in chunks of 64, the last one of 20: second trips of the row loops, where out_scale, da_scale and
#                                    the stage-slot writes of a solve had never run (tests/test_bnsolve_host.py asserts the regime)
GRIDS = [(0.0, 1.0), (0.0, 0.3, 0.55, 1.0), (1.0, 0.4, 0.0)]
E_FLOOR = {'out': 2e-6, 'gy': 2e-6, 'gp': 1.5e-3}


def shape_id(s):
    return 'n%d_c%d_%dx%d' % s


def grid_id(g):
    return 't' + '_'.join('%g' % v for v in g)


def inputs(shape, grid):
    y = torch.randn(*shape, generator=torch.Generator().manual_seed(4))
    wgt = torch.randn((len(grid),) + tuple(shape), generator=torch.Generator().manual_seed(7)) / y[0].numel() ** 0.5
    return y, wgt


def solve(mod, dev, odeint_adjoint, y, grid, tol, wgt, method, dtype=torch.float32):
    """One forward + backward solve: outputs, gradients, the function's NFE counter after either, the solver's statistics."""
    mod.nfe = 0
    for prm in mod.parameters():
        prm.grad = None
    y0 = y.detach().clone().to(device=dev, dtype=dtype).requires_grad_(True)
    out = odeint_adjoint(mod, y0, torch.tensor(grid, dtype=dtype).to(dev), rtol=tol, atol=tol, method=method)
    nfe_f = mod.nfe
    (out * wgt.to(device=dev, dtype=dtype)).sum().backward()
    return dict(out=out.detach().cpu(), gy=y0.grad.cpu(), gp=[None if p.grad is None else p.grad.cpu() for p in mod.parameters()],
                nfe=(nfe_f, mod.nfe), fwd=dict(getattr(mod, 'last_forward_stats', None) or {}),
                bwd=dict(getattr(mod, 'last_backward_stats', None) or {}))


@functools.lru_cache(maxsize=None)
def reference(shape, grid, kink_free, method, dtype=torch.float64):
    """The oracle's solve on the CPU copy of the function: computed once, shared, never modified."""
    from oracle import torchdiffeq_restated as tdq
    func, ref64 = B.func_pair(shape[1], SEED, kink_free)
    mod = ref64 if dtype == torch.float64 else copy.deepcopy(func)
    y, wgt = inputs(shape, grid)
    return solve(mod, 'cpu', tdq.odeint_adjoint, y, grid, 1e-3, wgt, method, dtype)


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-300))


def param_errors(got, ref):
    """Every parameter gradient against the reference's, each relative to max(its own scale, 1e-4 x the largest gradient of the
    function) -- the measure of tests/test_gpu_bnfunc.py::_grads_close; returns the largest."""
    gmax = max(float(r.abs().max()) for r in ref)
    worst = 0.0
    for g, r in zip(got, ref):
        g = torch.zeros_like(r) if g is None else g
        scale = max(float(r.abs().max()), 1e-4 * gmax)
        worst = max(worst, float((g.double() - r.double()).abs().max()) / scale)
    return worst


def errors(run, ref):
    return {'out': rel(run['out'], ref['out']), 'gy': rel(run['gy'], ref['gy']), 'gp': param_errors(run['gp'], ref['gp'])}

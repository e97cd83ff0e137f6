#!/usr/bin/env python
"""Forward + backward of the ResNet baseline's six-block residual trunk (resnet.py, csrc/trunk_api.hip) at the two
workload shapes, the fused node against the paths it replaces, in ONE process, alternating them round by round:

    python3 tools/resnet_time.py > profiles/resnet_trunk_time.txt

  fused      `ResidualTrunk.forward` on a HIP device: one autograd node, node_trunk_fwd / node_trunk_bwd
  modules    the same modules as a plain `nn.Sequential` (what the trunk runs for shapes the kernels refuse): MIOpen
             convolutions, the package's fused GroupNorm + ReLU launches (head.gn_relu), ATen additions
  aten       the same parameters through torch.nn.functional only: F.group_norm, F.relu, F.conv2d (MIOpen / ATen)

A timed call is a forward and `torch.autograd.grad` of the output with respect to the input and all 36 parameters, from
Python (what a training step sees: dispatch included).  HIP events around `--reps` calls, every path warmed up with 10
calls, the paths alternating round by round, median (and minimum) over `--rounds` rounds.  Input and cotangent ROTATE
through enough buffers to exceed the 256 MB Infinity Cache between two uses of one of them, so the operands are cache-cold.
`--kernels` instead runs a few fused steps at the first shape only, for a kernel trace taken around this script."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(128, 256, 8, 8), (128, 64, 7, 7)]      # CIFAR-10 and MNIST behind the residual stem (reproduce.sh)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=40)
    ap.add_argument('--rounds', type=int, default=9)
    ap.add_argument('--kernels', action='store_true')
    a = ap.parse_args()

    import torch
    import torch.nn.functional as F
    from torch import nn
    import neural_ode_features_amd as nof
    assert torch.cuda.is_available(), 'needs a HIP device'
    print('device: %s' % torch.cuda.get_device_name(0))

    for shape in SHAPES[:1] if a.kernels else SHAPES:
        n, c, h, w = shape
        torch.manual_seed(0)
        trunk = nof.ResidualTrunk(c, 6).cuda()
        params = list(trunk.parameters())
        nbytes = n * c * h * w * 4
        nsets = min(64, max(2, -(-320 * 1000 * 1000 // nbytes)))
        xs = [torch.randn(n, c, h, w, device='cuda').requires_grad_(True) for _ in range(nsets)]
        cots = [torch.randn(n, c, h, w, device='cuda') for _ in range(nsets)]

        def aten(x):
            for blk in trunk:
                a1 = F.relu(F.group_norm(x, blk.norm1.num_groups, blk.norm1.weight, blk.norm1.bias, blk.norm1.eps))
                hh = F.conv2d(a1, blk.conv1.weight, None, 1, 1)
                a2 = F.relu(F.group_norm(hh, blk.norm2.num_groups, blk.norm2.weight, blk.norm2.bias, blk.norm2.eps))
                x = F.conv2d(a2, blk.conv2.weight, None, 1, 1) + x
            return x
        paths = {'fused': trunk, 'modules': lambda x: nn.Sequential.forward(trunk, x), 'aten': aten}
        assert type(trunk(xs[0]).grad_fn).__name__ == '_TrunkFnBackward'

        def step_of(fwd):
            i = [0]

            def step():
                i[0] = (i[0] + 1) % nsets
                x = xs[i[0]]
                return torch.autograd.grad(fwd(x), [x] + params, cots[i[0]])
            return step

        if a.kernels:
            step = step_of(trunk)
            for _ in range(20):
                step()
            torch.cuda.synchronize()
            print('ran 20 fused steps at %s' % (shape,))
            continue

        # the paths compute the same thing: fused vs aten, worst gradient in relative L2 -- and in max norm with the GroupNorm
        # biases at +8 (kink-free: at 25 M pre-activations a few lie within fp32 rounding of zero, their ReLU masks differ
        # between any two fp32 implementations, and one flipped element moves a GroupNorm gradient by ~1 % of its largest entry)
        ga, gb = step_of(trunk)(), step_of(aten)()
        worst_l2 = max(float((u - v).norm() / v.norm()) for u, v in zip(ga, gb))
        with torch.no_grad():
            for blk in trunk:
                blk.norm1.bias.add_(8.0)
                blk.norm2.bias.add_(8.0)
        ga, gb = step_of(trunk)(), step_of(aten)()
        worst = max(float((u - v).abs().max() / v.abs().max()) for u, v in zip(ga, gb))
        with torch.no_grad():
            for blk in trunk:
                blk.norm1.bias.sub_(8.0)
                blk.norm2.bias.sub_(8.0)
        steps = {k: step_of(f) for k, f in paths.items()}
        for s in steps.values():
            for _ in range(10):
                s()
        torch.cuda.synchronize()

        def timed(step):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                step()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) * 1e3 / a.reps
        t = {k: [] for k in steps}
        for _ in range(a.rounds):
            for k, s in steps.items():
                t[k].append(timed(s))
        med = {k: statistics.median(v) for k, v in t.items()}
        print('\ntrunk of 6 blocks, x [%d, %d, %d, %d] (%.1f MB): forward + backward, input and 36 parameter gradients' % (n, c, h, w, nbytes / 1e6))
        print('%d calls per timed window, %d rounds, input and cotangent rotating through %d buffers (%.0f MB each way); '
              'fused vs aten gradients: worst relative L2 difference %.1e, kink-free worst max-norm difference %.1e of the largest entry'
              % (a.reps, a.rounds, nsets, nsets * nbytes / 1e6, worst_l2, worst))
        for k in steps:
            print('  %-8s median %9.1f us   min %9.1f us   max %9.1f us' % (k, med[k], min(t[k]), max(t[k])))
        print('  modules / fused %.2f, aten / fused %.2f' % (med['modules'] / med['fused'], med['aten'] / med['fused']))


if __name__ == '__main__':
    main()

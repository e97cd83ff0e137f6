#!/usr/bin/env python
"""The head of a whole trajectory [T, N, C, H, W] in one call (odenet.py `FCClassifier.forward`, `head_on_trajectory`; head.py
`bn_head_pool_slices`, `trajectory_loss`, `trajectory_distance`) against the loop over the slices and the chains of tensor operations
it replaces, in ONE process, alternating them round by round:

    python3 tools/traj_head_time.py > profiles/traj_head_time.txt

  one call   `FCClassifier.fused_trajectory = True`: the head's nodes on the flattened view (GroupNorm), node_bnhead_fwd_slices
             (BatchNorm), node_head_loss_slices_fwd, node_gn_relu_distance
  loop       the switch off: one head call per slice and a stack; the ATen chains of `evaluate accuracy` and `attack diff`

Timed calls, from Python (dispatch included), all under no_grad:
  the head of [21, 128, 256, 8, 8] and [21, 128, 64, 7, 7], pool only and with the Linear layer, GroupNorm and BatchNorm;
  the ResNet's head calls on the stem's output [128, 256, 8, 8] and the trunk's taps [6, 128, 256, 8, 8]: two against seven;
  `trajectory_loss` at [21, 128, 10] against the chain of `evaluate accuracy`, each with its read-back(s) to the host;
  `trajectory_distance` at [51, 128, 256, 8, 8] and [51, 1, 256, 8, 8] against the chain of `attack diff` from the same raw
    trajectories (the norm + ReLU slice by slice, stack, reshape, transpose, sub, pow, sum, sqrt, cosine_similarity), with the achieved
    TB/s of the 2 T N C H W 4 bytes the kernel must read;
  one `model(x)` of `evaluate features`: ODENet(3, 256 filters, residual stem) at [128, 3, 32, 32], tol 1e-3, 21 time points.
HIP events around `--reps` calls, every path warmed up, the paths alternating round by round, median, minimum and spread (max - min)
over `--rounds` rounds.  Operands ROTATE through enough buffers to exceed the 256 MB Infinity Cache between two uses of one of them.
The device kernels of ONE call are counted with torch.profiler in a run of its own (`--kernels`; the timed run does not trace).

A row is a GAIN when the loop's median minus the one call's median exceeds three times the spread of the loop's rounds of the same
run; a row whose one-call median is the larger one says SLOWER."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HEAD_SHAPES = [(21, 128, 256, 8, 8), (21, 128, 64, 7, 7)]
LOSS_SHAPE = (21, 128, 10)
DISTANCE_SHAPES = [(51, 128, 256, 8, 8), (51, 1, 256, 8, 8)]
HBM_ACHIEVABLE = 6.3e12       # bytes / s a streaming kernel reaches on an MI355X: the floor a read-once kernel is compared with


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--kernels', action='store_true', help='count the device kernels of one call of every path (no timing)')
    ap.add_argument('--no-model', action='store_true')
    a = ap.parse_args()

    import torch
    import torch.nn.functional as F
    import neural_ode_features_amd as nof
    from neural_ode_features_amd.odenet import FCClassifier, head_on_trajectory
    assert torch.cuda.is_available(), 'needs a HIP device'
    print('device: %s' % torch.cuda.get_device_name(0))

    def switched(on, fn):
        def call(*args):
            FCClassifier.fused_trajectory = on
            try:
                return fn(*args)
            finally:
                FCClassifier.fused_trajectory = True
        return call

    def timed(step, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            step()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / reps

    def kernels_of(step):
        try:
            from torch.autograd import DeviceType
            from torch.profiler import ProfilerActivity, profile
            torch.cuda.synchronize()
            with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
                step()
                torch.cuda.synchronize()
            return sum(e.count for e in prof.key_averages() if e.device_type == DeviceType.CUDA)
        except Exception as exc:      # (no device tracing in this build)
            return 'n/a (%s)' % type(exc).__name__

    def compare(what, one, loop, reps, rounds, unit=1.0, suffix='us', warm=5, nbytes=None):
        steps = {'one call': one, 'loop': loop}
        for s in steps.values():
            for _ in range(warm):
                s()
        torch.cuda.synchronize()
        if a.kernels:
            print('  %-34s device kernels per call: one call %s, loop %s' % (what, kernels_of(one), kernels_of(loop)), flush=True)
            return
        ts = {k: [] for k in steps}
        for _ in range(rounds):
            for k, s in steps.items():
                ts[k].append(timed(s, reps) / unit)
        med = {k: statistics.median(v) for k, v in ts.items()}
        spread = {k: max(v) - min(v) for k, v in ts.items()}
        for k in steps:
            extra = ''
            if nbytes is not None and k == 'one call':
                secs = med[k] * unit * 1e-6
                extra = '   %.2f TB/s of the %.1f MB it must read (at %.1f TB/s: %.1f us)' % (nbytes / secs / 1e12, nbytes / 1e6, HBM_ACHIEVABLE / 1e12,
                                                                                              nbytes / HBM_ACHIEVABLE * 1e6)
            print('  %-34s %-8s median %9.2f %s   min %9.2f   spread %8.2f%s' % (what, k, med[k], suffix, min(ts[k]), spread[k], extra))
        diff = med['loop'] - med['one call']
        verdict = 'GAIN' if diff > 3 * spread['loop'] else ('SLOWER one call' if diff < 0 else 'no gain by the bar')
        print('  %-34s loop / one call %.2f   difference of the medians %.2f %s against 3 x the loop\'s spread %.2f: %s'
              % (what, med['loop'] / med['one call'], diff, suffix, 3 * spread['loop'], verdict), flush=True)

    def sets_for(nbytes):
        return min(64, max(2, -(-320 * 1000 * 1000 // nbytes)))

    torch.set_grad_enabled(False)

    # -----------------------------------------------------------------------------------------------------------------
    # the head of a trajectory
    # -----------------------------------------------------------------------------------------------------------------
    for shape in HEAD_SHAPES:
        t, n, c, h, w = shape
        nsets = sets_for(4 * t * n * c * h * w)
        trajs = [torch.randn(*shape, device='cuda') for _ in range(nsets)]
        print('\nhead of a trajectory [%d, %d, %d, %d, %d] (%.0f MB, %d of them in turn); %d calls per timed window, %d rounds'
              % (t, n, c, h, w, trajs[0].numel() * 4 / 1e6, nsets, a.reps, a.rounds))
        for norm in ('group', 'batch'):
            for linear in (False, True):
                torch.manual_seed(0)
                head = FCClassifier(in_ch=c, out=10, norm=norm).cuda().eval()
                if not linear:
                    head.module[-1] = torch.nn.Sequential()
                i = [0]

                def call():
                    i[0] = (i[0] + 1) % nsets
                    return head(trajs[i[0]])
                i[0] = 0
                ya = switched(True, call)()
                i[0] = 0
                yb = switched(False, call)()
                assert torch.equal(ya, yb), (shape, norm, linear)
                compare('%s norm, %s' % (norm, 'with Linear' if linear else 'pool only'), switched(True, call), switched(False, call),
                        a.reps, a.rounds)
        del trajs
        torch.cuda.empty_cache()

    # -----------------------------------------------------------------------------------------------------------------
    # the ResNet's head calls: stem output + taps
    # -----------------------------------------------------------------------------------------------------------------
    n, c, h, w = 128, 256, 8, 8
    nsets = sets_for(4 * 7 * n * c * h * w)
    xs = [torch.randn(n, c, h, w, device='cuda') for _ in range(nsets)]
    taps = [torch.randn(6, n, c, h, w, device='cuda') for _ in range(nsets)]
    print('\nResNet feature extraction, the head on the stem\'s output [%d, %d, %d, %d] and the trunk\'s taps [6, %d, %d, %d, %d] '
          '(%d sets in turn): two head calls and a cat against seven and a stack' % (n, c, h, w, n, c, h, w, nsets))
    for norm in ('group', 'batch'):
        torch.manual_seed(0)
        head = FCClassifier(in_ch=c, out=10, norm=norm).cuda().eval()
        head.module[-1] = torch.nn.Sequential()
        i = [0]

        def two_calls():
            i[0] = (i[0] + 1) % nsets
            return torch.cat([head_on_trajectory(head, xs[i[0]].unsqueeze(0)), head_on_trajectory(head, taps[i[0]])])

        def seven_calls():
            i[0] = (i[0] + 1) % nsets
            return torch.stack([head(f) for f in [xs[i[0]]] + list(taps[i[0]].unbind(0))])
        i[0] = 0
        ya = two_calls()
        i[0] = 0
        assert torch.equal(ya, seven_calls())
        compare('%s norm, pool only' % norm, two_calls, seven_calls, a.reps, a.rounds)
    del xs, taps
    torch.cuda.empty_cache()

    # -----------------------------------------------------------------------------------------------------------------
    # the loss of the accuracy sweep
    # -----------------------------------------------------------------------------------------------------------------
    t, n, o = LOSS_SHAPE
    logits = [torch.randn(t, n, o, device='cuda') for _ in range(8)]
    target = torch.randint(0, o, (n,), device='cuda')
    i = [0]

    def sliced_loss():
        i[0] = (i[0] + 1) % 8
        return nof.trajectory_loss(logits[i[0]], target).cpu()

    def aten_loss():
        i[0] = (i[0] + 1) % 8
        pr = logits[i[0]]
        losses = F.cross_entropy(pr.permute(1, 2, 0), target.unsqueeze(1).expand(-1, t), reduction='none')
        return losses.sum(0).cpu(), (target.unsqueeze(0).expand(t, -1) == pr.argmax(dim=-1)).sum(-1).float().cpu()
    print('\nloss and hits of every slice, logits [%d, %d, %d], read back to the host as `evaluate accuracy` does (one read-back against two)' % LOSS_SHAPE)
    compare('trajectory_loss', sliced_loss, aten_loss, a.reps, a.rounds)

    # -----------------------------------------------------------------------------------------------------------------
    # the trajectory distance of `attack diff`
    # -----------------------------------------------------------------------------------------------------------------
    for shape in DISTANCE_SHAPES:
        t, n, c, h, w = shape
        nbytes = 2 * 4 * t * n * c * h * w
        nsets = 1 if nbytes > 320e6 else sets_for(nbytes)       # (a call that reads more than the cache holds evicts its own operands)
        pairs = [(torch.randn(*shape, device='cuda'),) for _ in range(nsets)]
        pairs = [(p[0], p[0] + 0.05 * torch.randn(*shape, device='cuda')) for p in pairs]
        torch.manual_seed(0)
        gn = torch.nn.GroupNorm(min(32, c), c).cuda()
        act = torch.nn.Sequential(gn, torch.nn.ReLU(inplace=True))
        i = [0]

        def kernel():
            i[0] = (i[0] + 1) % nsets
            return nof.trajectory_distance(pairs[i[0]][0], pairs[i[0]][1], gn)

        def chain():
            i[0] = (i[0] + 1) % nsets
            u0 = torch.stack([act(v) for v in pairs[i[0]][0]]).reshape(t, n, -1).transpose(0, 1)
            u1 = torch.stack([act(v) for v in pairs[i[0]][1]]).reshape(t, n, -1).transpose(0, 1)
            return (u1 - u0).pow(2).sum(-1).sqrt(), F.cosine_similarity(u1, u0, dim=-1)
        i[0] = 0
        l2a, cosa = kernel()
        i[0] = 0
        l2b, cosb = chain()
        print('\ntrajectory distance, two raw trajectories [%d, %d, %d, %d, %d] (%.1f MB each, %d pair(s) in turn); kernel against chain: worst '
              'relative difference of l2 %.1e, worst difference of cos %.1e'
              % (t, n, c, h, w, nbytes / 2e6, nsets, float(((l2a - l2b.t()) / l2b.t()).abs().max()), float((cosa - cosb.t()).abs().max())))
        del l2a, cosa, l2b, cosb
        big = nbytes > 320e6
        compare('trajectory_distance', kernel, chain, max(2, a.reps // 4) if big else a.reps, a.rounds, unit=1e3 if big else 1.0,
                suffix='ms' if big else 'us', warm=2 if big else 5, nbytes=nbytes)
        del pairs
        torch.cuda.empty_cache()

    if a.no_model:
        return
    # -----------------------------------------------------------------------------------------------------------------
    # one model(x) of `evaluate features`
    # -----------------------------------------------------------------------------------------------------------------
    torch.manual_seed(0)
    model = nof.ODENet(3, n_filters=256, downsample='residual', adjoint=True, tol=1e-3, method='dopri5').cuda().eval()
    model.to_features_extractor()
    model.odeblock.t1 = [0.05 * k for k in range(1, 21)]
    images = [torch.randn(128, 3, 32, 32, device='cuda') for _ in range(4)]
    i = [0]

    def features():
        i[0] = (i[0] + 1) % 4
        return model(images[i[0]])
    i[0] = 0
    ya = switched(True, features)()
    i[0] = 0
    yb = switched(False, features)()
    assert ya.shape == (21, 128, 256) and torch.equal(ya, yb)
    print('\none model(x) of `evaluate features`: ODENet(3, 256 filters, residual stem, dopri5 tol 1e-3), x [128, 3, 32, 32], 21 time points')
    compare('model(x), features', switched(True, features), switched(False, features), a.reps, a.rounds, unit=1e3, suffix='ms', warm=3)


if __name__ == '__main__':
    main()

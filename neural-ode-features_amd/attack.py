#!/usr/bin/env python
"""Basic-iterative (BIM / PGD) adversarial attacks on the nets of this package -- the third paper the reference reproduces,
*On the robustness to adversarial examples of neural ODE image classifiers* (`/root/reference/adversarial/attack.py`,
`adversarial/diff.py`, `adversarial/reproduce.sh`).

    bim(model, images, labels, norm=inf | 2, epsilon=..., stepsize=..., iterations=10, return_early=True,
        bounds=(0, 1), preprocessing=(mean, std))  ->  BimResult(adversarial, distance, adversarial_class, original_class,
                                                                  found_iteration)

Semantics: foolbox 2.x's `LinfinityBasicIterativeAttack` / `L2BasicIterativeAttack` as attack.py:72 calls them
(`binary_search=False`, no random start, untargeted, `Misclassification`).  With s = hi - lo, per sample:

  1. evaluate x0; already misclassified (a "natural error", diff.py:90): distance 0, adversarial_class = the prediction,
     never stepped;
  2. `iterations` times: g = d CE(logits, label) / dx (through the preprocessing), then
         Linf:  x += stepsize * sign(g) * s;                     p = clip(x - x0, -eps s, eps s)
         L2:    x += stepsize * g / max(1e-12, rms(g)) * s;      p = (x - x0) * min(1, eps s / max(1e-12, rms(x - x0)))
         x = clip(x0 + p, lo, hi)            (rms: root MEAN square)
     evaluate x; misclassified: record class, iteration and distance (mean((x - x0)^2) / s^2 for L2, max |x - x0| / s for
     Linf) and, with `return_early`, stop this sample; without it the sample goes on and the smallest distance is kept;
  3. never found: distance inf, class -1; `adversarial` then holds the last iterate.

One forward per iteration serves the check of iteration k and the gradient of iteration k + 1: `iterations + 1` forwards (the
last without a graph) and `iterations` backwards (foolbox: twice the forwards).  The loss is the sum-reduced cross entropy, so
each sample's gradient is its own; a batch shares dopri5's step sequence, as everywhere in this package (batch size 1
reproduces the reference's per-image solves).

fp32 images on a HIP device run the library's path: parameters frozen for the duration (the `residual`, `convolution` and
`minimal` stems then run their data-gradient chains alone -- the `input_grad` switch of `ResidualStem`, `ConvStem` and
`MinimalStem`: node_stem_bwd_dx, node_convstem_bwd_dx, node_ministem_bwd -- so an attack on a run of any of the three goes
through the fused stem with no library convolution in it), the fused loss, and two launches per iteration for
the attack's own arithmetic (node_attack_step, node_attack_judge; csrc/kernels_attack.hip).  Anything else -- CPU tensors,
fp64, any callable model -- runs `bim_reference`, the same loop in plain torch, which is also what the tests compare against.

Command line (run loading as `evaluate.load_run`; the test images must be the UNNORMALISED ones, uint8 or floats in [0, 1]:
the attack applies `PREPROC[dataset]` itself, attack.py:26-32):

    python -m neural_ode_features_amd.attack attack RUN -t TOL -e EPS -d {inf,2} -s STEP [--batch-size B] [--limit N]
    python -m neural_ode_features_amd.attack diff   RUN -t TOL -e EPS -d {inf,2} -s STEP [-r RESOLUTION]

  attack  -> RUN/adv-attack/<tol,eps,distance,stepsize>/results.csv with the reference's columns sample_id, label,
             elapsed_time, distance, adversarial_class, original_class; samples already in the file are skipped
  diff    for every sample of results.csv with a finite, non-zero distance: the attack again, then the trajectories of the
          original and of the adversarial image through a second model in `to_features_extractor(keep_pool=False)` mode with
          `odeblock.t1 = linspace(0, 1, resolution + 1)` -> diff_l2.csv, diff_cos.csv (columns sample_id, t...): the L2 norm
          of the difference and the cosine similarity per time point.

Two deliberate departures from diff.py: line 97 forgets to pass `stepsize` and silently attacks with foolbox's default 0.05
-- here `diff` attacks with `-s`, like `attack`; and lines 105-109 feed the extractor the un-normalised pixels although
the model was trained on and attacked through normalised ones -- here the extractor sees what the model sees.
"""
from __future__ import annotations

import argparse
import collections
import contextlib
import ctypes as C
import math
import os
import time

import torch
import torch.nn.functional as F

BimResult = collections.namedtuple('BimResult', 'adversarial distance adversarial_class original_class found_iteration')

INF = float('inf')
COLUMNS = ('sample_id', 'label', 'elapsed_time', 'distance', 'adversarial_class', 'original_class')


def _norm_kind(norm):
    if norm in (INF, 'inf'):
        return INF
    if norm in (2, 2.0, '2'):
        return 2
    raise ValueError('norm=%r: float("inf") or 2' % (norm,))


def _stats(preprocessing, like, channels):
    """(mean, std) as [1, C, 1, 1] tensors like `like`, or (None, None)."""
    if preprocessing is None:
        return None, None
    mean, std = preprocessing
    mean = torch.as_tensor(mean, dtype=like.dtype, device=like.device).reshape(1, -1, 1, 1)
    std = torch.as_tensor(std, dtype=like.dtype, device=like.device).reshape(1, -1, 1, 1)
    if mean.shape[1] not in (1, channels) or std.shape[1] not in (1, channels) or bool((std <= 0).any()):
        raise ValueError('preprocessing: mean and std hold one entry per channel, std > 0')
    return mean.expand(1, channels, 1, 1), std.expand(1, channels, 1, 1)


def _rms(v):
    return v.flatten(1).pow(2).mean(1).sqrt().reshape(-1, 1, 1, 1)


def step_reference(x, x0, g, norm, stepsize, epsilon, bounds=(0, 1)):
    """One iteration's update in plain torch: `g` is the gradient with respect to the pixels `x`; returns the new x."""
    lo, hi = bounds
    s = hi - lo
    if _norm_kind(norm) == INF:
        x1 = x + stepsize * (g.sign() * s)
        p = (x1 - x0).clamp(-epsilon * s, epsilon * s)
    else:
        x1 = x + stepsize * (g * (s / _rms(g).clamp_min(1e-12)))
        d = x1 - x0
        p = d * (epsilon * s / _rms(d).clamp_min(1e-12)).clamp_max(1.0)
    return (x0 + p).clamp(lo, hi)


def distance_reference(x, x0, norm, bounds=(0, 1)):
    """foolbox's MeanSquaredDistance (L2) / Linfinity, per sample."""
    s = bounds[1] - bounds[0]
    d = (x - x0).flatten(1)
    if _norm_kind(norm) == INF:
        return d.abs().max(1).values / s
    return d.pow(2).mean(1) / (s * s)


def bim_reference(model, images, labels, *, norm=INF, epsilon, stepsize, iterations=10, return_early=True, bounds=(0, 1),
                  preprocessing=None):
    """The attack in plain torch with any callable `model` (normalised images -> logits), on the images' device and dtype."""
    norm = _norm_kind(norm)
    n = images.shape[0]
    dev = images.device
    x0 = images.detach().clone()
    x = x0.clone()
    mean, std = _stats(preprocessing, x0, x0.shape[1])
    labels = labels.to(dev)
    active = torch.ones(n, dtype=torch.bool, device=dev)
    distance = torch.full((n,), INF, dtype=x0.dtype, device=dev)
    adv_class = torch.full((n,), -1, dtype=torch.int64, device=dev)
    found = torch.full((n,), -1, dtype=torch.int64, device=dev)
    best = x0.clone()
    original = None
    for k in range(iterations + 1):
        xg = x.detach().clone().requires_grad_(k < iterations)
        with torch.enable_grad() if k < iterations else torch.no_grad():
            logits = model((xg - mean) / std if mean is not None else xg)
            pred = logits.detach().argmax(1)
            wrong = pred != labels
            if k == 0:
                original = pred.clone()
                hit = wrong
                dist = torch.zeros_like(distance)
            else:
                dist = distance_reference(x, x0, norm, bounds)
                hit = wrong & active & (dist < distance if not return_early else torch.ones_like(wrong))
            distance = torch.where(hit, dist, distance)
            adv_class = torch.where(hit, pred, adv_class)
            found = torch.where(hit, torch.full_like(found, k), found)
            best = torch.where(hit.reshape(-1, 1, 1, 1), x, best)
            if k == 0 or return_early:
                active = active & ~hit
            if k == iterations or not bool(active.any()):
                break
            g, = torch.autograd.grad(F.cross_entropy(logits, labels, reduction='sum'), xg)
        xnew = step_reference(x, x0, g.detach(), norm, stepsize, epsilon, bounds)
        x = torch.where(active.reshape(-1, 1, 1, 1), xnew, x)
    adversarial = torch.where((found >= 0).reshape(-1, 1, 1, 1), best, x)
    return BimResult(adversarial, distance, adv_class, original, found)


@contextlib.contextmanager
def _frozen(model, fused_stem):
    """Parameters without gradients and the fused stems (residual, convolution, minimal) on their input-gradient path for the
    duration."""
    from .convstem import ConvStem
    from .ministem import MinimalStem
    from .stem import ResidualStem
    params = [p for p in model.parameters() if p.requires_grad]
    stems = [(m, m.input_grad) for m in model.modules() if isinstance(m, (ResidualStem, ConvStem, MinimalStem))]
    for p in params:
        p.requires_grad_(False)
    for m, _ in stems:
        m.input_grad = bool(fused_stem)
    try:
        yield
    finally:
        for p in params:
            p.requires_grad_(True)
        for m, was in stems:
            m.input_grad = was


def _bim_hip(model, images, labels, norm, epsilon, stepsize, iterations, return_early, bounds, preprocessing, fused_stem):
    from . import _lib
    from .head import cross_entropy
    lib = _lib.load()
    dev = images.device
    n, c, h, w = images.shape
    x0 = images.detach().contiguous().clone()
    x = x0.clone()
    labels = labels.to(dev, torch.int64).contiguous()
    mean, std = _stats(preprocessing, x0, c)
    if mean is not None:
        mean_d, std_d = mean.reshape(-1).contiguous(), std.reshape(-1).contiguous()
        xn = ((x - mean) / std).contiguous()
    else:
        mean_d = std_d = None
        xn = x.clone()
    active = torch.ones(n, dtype=torch.int32, device=dev)
    original = torch.full((n,), -1, dtype=torch.int32, device=dev)
    adv_class = torch.full((n,), -1, dtype=torch.int32, device=dev)
    found = torch.full((n,), -1, dtype=torch.int32, device=dev)
    distance = torch.full((n,), INF, dtype=torch.float32, device=dev)
    best = torch.empty_like(x0) if not return_early else None
    atk = _lib.NodeAttack(n, c, h, w, _lib.ATTACK_LINF if norm == INF else _lib.ATTACK_L2, int(bool(return_early)),
                          float(stepsize), float(epsilon), float(bounds[0]), float(bounds[1]),
                          mean_d.data_ptr() if mean_d is not None else None, std_d.data_ptr() if std_d is not None else None)
    rec = _lib.NodeAttackRecord(active.data_ptr(), original.data_ptr(), adv_class.data_ptr(), found.data_ptr(), distance.data_ptr(),
                                best.data_ptr() if best is not None else None)
    with _frozen(model, fused_stem), torch.cuda.device(dev):
        for k in range(iterations + 1):
            last = k == iterations
            xin = xn.detach().requires_grad_(not last)
            with torch.no_grad() if last else torch.enable_grad():
                logits = model(xin)
                if logits.dim() != 2 or logits.shape[0] != n:
                    raise ValueError('the model must return [n, classes] logits (got %s)' % (tuple(logits.shape),))
                lg = logits.detach().float().contiguous()
                stream = torch.cuda.current_stream(dev).cuda_stream
                _lib.check(lib.node_attack_judge(C.byref(atk), lg.shape[1], lg.data_ptr(), labels.data_ptr(), x.data_ptr(),
                                                 x0.data_ptr(), int(k == 0), k, C.byref(rec), stream))
                if last:
                    break
                if return_early and not bool(active.any()):       # (4 bytes per iteration, against a forward and an adjoint solve)
                    break
                g, = torch.autograd.grad(cross_entropy(logits, labels, reduction='sum'), xin)
            g = g.contiguous()
            _lib.check(lib.node_attack_step(C.byref(atk), x.data_ptr(), x0.data_ptr(), g.data_ptr(), active.data_ptr(),
                                            xn.data_ptr(), stream))
    hit = found >= 0
    if best is not None:
        adversarial = torch.where(hit.reshape(-1, 1, 1, 1), best, x)
    else:
        adversarial = x
    return BimResult(adversarial, distance, adv_class.long(), original.long(), found.long())


def bim(model, images, labels, *, norm=INF, epsilon, stepsize, iterations=10, return_early=True, bounds=(0, 1),
        preprocessing=None, fused_stem=True):
    """The basic-iterative attack on a batch (module docstring).  `model`: normalised images -> logits; `images`: [n, C, H, W]
    in pixel space `bounds`; `preprocessing`: (mean, std) per channel, or None.  `fused_stem=False` keeps a residual,
    convolution or minimal stem on the module sequence (its default for inputs that require a gradient)."""
    norm = _norm_kind(norm)
    if images.dim() != 4 or labels.shape[0] != images.shape[0]:
        raise ValueError('images [n, C, H, W] and labels [n]')
    if not bounds[1] > bounds[0] or epsilon < 0 or stepsize < 0 or iterations < 0:
        raise ValueError('bounds (lo < hi), epsilon >= 0, stepsize >= 0, iterations >= 0')
    if images.is_cuda and images.dtype == torch.float32 and isinstance(model, torch.nn.Module):
        return _bim_hip(model, images, labels, norm, epsilon, stepsize, iterations, return_early, bounds, preprocessing, fused_stem)
    return bim_reference(model, images, labels, norm=norm, epsilon=epsilon, stepsize=stepsize, iterations=iterations,
                         return_early=return_early, bounds=bounds, preprocessing=preprocessing)


# ---------------------------------------------------------------------------------------------------------------------
# command line
# ---------------------------------------------------------------------------------------------------------------------
def sub_dir(run, tol, epsilon, distance, stepsize):
    """RUN/adv-attack/<tol,eps,distance,stepsize>: one folder per setting of the sweep (reproduce.sh)."""
    return os.path.join(run, 'adv-attack', 'tol=%g,eps=%g,distance=%g,stepsize=%g' % (tol, epsilon, distance, stepsize))


def read_results(path):
    """results.csv -> {sample_id: row dict}; a missing file is an empty table."""
    import pandas as pd
    if not os.path.exists(path):
        return {}
    df = pd.read_csv(path)
    return {int(r['sample_id']): r for r in df.to_dict('records')}


def append_rows(path, rows, columns=COLUMNS):
    """Append `rows` (dicts) to the csv at `path`, writing the header when the file is new."""
    import pandas as pd
    if not rows:
        return
    new = not os.path.exists(path)
    pd.DataFrame(rows, columns=list(columns)).to_csv(path, mode='w' if new else 'a', header=new, index=False)


def pending(n, done):
    """The sample ids of range(n) that `done` (ids already in results.csv) does not hold."""
    return [i for i in range(n) if i not in done]


def unit_images(x):
    """The test images in [0, 1]: uint8 / 255, floats as they are (they must already lie in [0, 1])."""
    if x.dtype == torch.uint8:
        return x.float() / 255
    x = x.float()
    if x.numel() and (float(x.min()) < 0 or float(x.max()) > 1):
        raise SystemExit('the attack works in pixel space [0, 1] and normalises itself: the test images must be uint8 or floats '
                         'in [0, 1] (they span [%g, %g])' % (float(x.min()), float(x.max())))
    return x


def _load(args):
    """(model, params, images in [0, 1], labels, preprocessing)."""
    from .augment import PREPROC
    import types
    from .train import load_data
    model, p = load_run_raw(args.run)
    if getattr(p, 'data', None):
        blob = torch.load(p.data, map_location='cpu')
        xte, yte = blob['x_test'], blob['y_test']
    else:
        q = types.SimpleNamespace(**vars(p))
        q.augmentation = 'crop'          # the synthetic set as 8-bit images (train.load_data)
        _, _, xte, yte, _, _ = load_data(q)
    xte = unit_images(xte)
    if args.limit:
        xte, yte = xte[:args.limit], yte[:args.limit]
    pre = PREPROC.get(p.dataset)
    if args.tol is None:
        args.tol = p.tol
    return model, p, xte, yte, pre


def load_run_raw(run_dir, which='best'):
    """`evaluate.load_run` without its test transform: the model and its params (the attack normalises the raw pixels itself)."""
    import types
    from .resnet import build_model
    from .train import SHAPES
    path = os.path.join(run_dir, which + '.pth')
    if not os.path.exists(path):
        path = os.path.join(run_dir, 'last.pth')
    ckpt = torch.load(path, map_location='cpu', weights_only=False)
    p = types.SimpleNamespace(**ckpt['params'])
    if getattr(p, 'data', None):
        blob = torch.load(p.data, map_location='cpu')
        in_ch, out = blob['x_test'].shape[1], int(blob['y_train'].max()) + 1
    else:
        in_ch, _, out = SHAPES[p.dataset]
    model = build_model(p, in_ch, out)
    model.load_state_dict(ckpt['model'])
    return model, p


def _set_tol(model, p, tol):
    if getattr(p, 'model', 'odenet') != 'resnet':
        model.odeblock.tol = tol


def attack(args):
    """attack.py:16-91, a batch at a time."""
    model, p, xte, yte, pre = _load(args)
    model = model.to(args.device).eval()
    _set_tol(model, p, args.tol)
    out_dir = sub_dir(args.run, args.tol, args.epsilon, args.distance, args.stepsize)
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, 'results.csv')
    todo = pending(xte.shape[0], read_results(path))
    print('%s: %d samples to attack, %d already there' % (path, len(todo), xte.shape[0] - len(todo)))
    for i in range(0, len(todo), args.batch_size):
        ids = todo[i:i + args.batch_size]
        x, y = xte[ids].to(args.device), yte[ids].to(args.device)
        start = time.time()
        r = bim(model, x, y, norm=args.distance, epsilon=args.epsilon, stepsize=args.stepsize, iterations=args.iterations,
                preprocessing=pre)
        dist, adv, orig = r.distance.cpu(), r.adversarial_class.cpu(), r.original_class.cpu()
        elapsed = (time.time() - start) / len(ids)
        append_rows(path, [dict(sample_id=s, label=int(yte[s]), elapsed_time=elapsed, distance=float(dist[j]),
                                adversarial_class=int(adv[j]) if int(adv[j]) >= 0 else float('nan'), original_class=int(orig[j]))
                           for j, s in enumerate(ids)])
    return path


def _diff_fused(extractor, x):
    """`diff`'s two numbers per time point from `head.trajectory_distance`'s kernel: a HIP fp32 batch through an extractor whose
    stem is no ODE stem (those return a tuple) and whose head, after `to_features_extractor(keep_pool=False)`, is an affine
    GroupNorm + ReLU without hooks.  `FCClassifier.fused_trajectory = False`: the chain of tensor operations, as before."""
    from .odenet import FCClassifier, ODEDownsample, ODEDownsample2
    head = extractor.classifier
    return (FCClassifier.fused_trajectory and x.is_cuda and x.dtype == torch.float32
            and not isinstance(extractor.downsample, (ODEDownsample, ODEDownsample2))
            and isinstance(head, torch.nn.Sequential) and len(head) == 2 and isinstance(head[0], torch.nn.GroupNorm)
            and head[0].affine and isinstance(head[1], torch.nn.ReLU)
            and not any(m._forward_hooks or m._forward_pre_hooks for m in (extractor, head, head[0], head[1])))


def diff(args):
    """diff.py:18-127."""
    import numpy as np
    from .head import trajectory_distance
    model, p, xte, yte, pre = _load(args)
    if getattr(p, 'model', 'odenet') == 'resnet':
        raise SystemExit('attack diff compares trajectories of the ODE block: the run is a ResNet')
    extractor = load_run_raw(args.run)[0].to(args.device).eval()
    extractor.to_features_extractor(keep_pool=False)
    t = np.linspace(0, 1, args.resolution + 1).tolist()
    extractor.odeblock.t1 = t
    model = model.to(args.device).eval()
    _set_tol(model, p, args.tol)
    extractor.odeblock.tol = args.tol
    out_dir = sub_dir(args.run, args.tol, args.epsilon, args.distance, args.stepsize)
    path = os.path.join(out_dir, 'results.csv')
    if not os.path.exists(path):
        raise SystemExit('no results of an attack found: %s' % path)
    results = read_results(path)
    l2_path, cos_path = os.path.join(out_dir, 'diff_l2.csv'), os.path.join(out_dir, 'diff_cos.csv')
    done = set(read_results(l2_path)) & set(read_results(cos_path))
    todo = [i for i in range(xte.shape[0]) if i in results and i not in done
            and results[i]['distance'] != 0 and math.isfinite(results[i]['distance'])]
    cols = ['sample_id'] + [repr(v) for v in t]
    mean, std = _stats(pre, xte[:1].to(args.device), xte.shape[1])
    for i in range(0, len(todo), args.batch_size):
        ids = todo[i:i + args.batch_size]
        x, y = xte[ids].to(args.device), yte[ids].to(args.device)
        r = bim(model, x, y, norm=args.distance, epsilon=args.epsilon, stepsize=args.stepsize, iterations=args.iterations,
                preprocessing=pre)
        ok = (r.found_iteration > 0).cpu()
        with torch.no_grad():
            a, b = ((v - mean) / std if mean is not None else v for v in (x, r.adversarial))
            if _diff_fused(extractor, a):
                # the RAW trajectories into one launch that normalises both in registers and writes neither (head.trajectory_distance)
                l2, cos = trajectory_distance(extractor.odeblock(extractor.downsample(a)),
                                              extractor.odeblock(extractor.downsample(b)), extractor.classifier[0])
                l2, cos = l2.t().cpu(), cos.t().cpu()
            else:
                traj0 = extractor(a)       # [T, n, C, H, W]
                traj1 = extractor(b)
                T = traj0.shape[0]
                traj0 = traj0.reshape(T, len(ids), -1).transpose(0, 1)
                traj1 = traj1.reshape(T, len(ids), -1).transpose(0, 1)
                l2 = (traj1 - traj0).pow(2).sum(-1).sqrt().cpu()
                cos = F.cosine_similarity(traj1, traj0, dim=-1).cpu()
        rows_l2, rows_cos = [], []
        for j, s in enumerate(ids):
            if not bool(ok[j]):
                print('WARN: adversarial not found when reproducing [sample_id = %d]' % s)
                continue
            rows_l2.append(dict(zip(cols, [s] + l2[j].tolist())))
            rows_cos.append(dict(zip(cols, [s] + cos[j].tolist())))
        append_rows(l2_path, rows_l2, cols)
        append_rows(cos_path, rows_cos, cols)
    return l2_path, cos_path


def _distance(text):
    v = float(text)
    if v not in (2.0, INF):
        raise argparse.ArgumentTypeError('2 or inf')
    return v


def build_parser():
    ap = argparse.ArgumentParser(description='basic-iterative adversarial attacks on a trained run (adversarial/attack.py, diff.py)')
    ap.add_argument('mode', choices=('attack', 'diff'))
    ap.add_argument('run', help='run directory to attack')
    ap.add_argument('-t', '--tol', type=float, default=None, help='ODE solver tolerance (default: the run\'s)')
    ap.add_argument('-e', '--epsilon', type=float, default=0.3, help='maximum perturbation allowed')
    ap.add_argument('-d', '--distance', type=_distance, default=INF, help='L_p distance: inf or 2')
    ap.add_argument('-s', '--stepsize', type=float, default=0.05, help='step size')
    ap.add_argument('-i', '--iterations', type=int, default=10)
    ap.add_argument('-r', '--resolution', type=int, default=50, help='diff: number of sampling intervals of the trajectory')
    ap.add_argument('--batch-size', type=int, default=128, help='images per solve (1: the reference\'s per-image solves)')
    ap.add_argument('--limit', type=int, default=0, help='only the first N test images')
    return ap


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.batch_size < 1:
        raise SystemExit('--batch-size must be >= 1')
    if not torch.cuda.is_available():
        raise SystemExit('neural_ode_features_amd.attack needs a HIP device: the ODE block has no CPU path')
    args.device = torch.device('cuda')
    return {'attack': attack, 'diff': diff}[args.mode](args)


if __name__ == '__main__':
    main()

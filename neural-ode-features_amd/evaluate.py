#!/usr/bin/env python
"""The evaluations of the reference that drive the ODE block, on the HIP backend
(`/root/reference/evaluate.py:24-305`; the second-heaviest user of the path):

  features   `model.to_features_extractor()`, `odeblock.t1 = [0, .05, ..., 1]`, `odeblock.tol` swept: one dense-output
             solve per batch and tolerance, the head's pooling per time slice  -> features [tols, T, N, C]
             (evaluate.py:24-94; written as .npz -- h5py is not in this image)
  nfe        batch size 1, `tol x t1` sweep, `model.nfe(reset=True)` per image -> nfe.csv.gz with the reference's
             columns y_true, y_pred, nfe, t1, tol (evaluate.py:97-142): the latency regime
  tradeoff   `tol x t1` sweep at the run's batch size, `odeblock.t1` / `.tol` mutated between forwards: test loss, accuracy and
             mean NFE per batch -> tradeoff.csv with the reference's columns t1, test_loss, test_acc, test_nfe, test_tol
             (evaluate.py:145-204)
  accuracy   ONE dense-output solve per batch and tolerance at t1 = [.05, ..., 1] (`return_last_only = False`; the ODE stem of an
             `ode2` run alike, `apply_conv = True`): loss and accuracy of the classifier at EVERY time slice -> `results` (csv)
             with the reference's columns t1, test_loss, test_acc, test_nfe, test_tol (evaluate.py:207-305)
  retrieval  reads the `features` mode's features.npz: per tolerance slice, per t1 slice, every test image as a query against
             the test set (database at the last slice 'asym' and at the query's own slice 'sym'), AP and AP@10 on the HIP
             scoring / ranking kernels (retrieval.py) -> retrieval.csv with the reference's columns ap_asym, ap_sym, ap10_asym,
             ap10_sym, t1, plus tol (evaluate.py:308-361)
  finetune   reads features.npz too: per tolerance slice, per t1 slice (or, with -a / --aggregate, their mean over t1 as one
             slice t1 = -1), `GridSearchCV(LinearSVC(), C = logspace(-2, 2, 5), cv=5)` as one batch of SVM problems on the HIP
             solver (finetune.py) -> finetune.csv with the reference's columns block, t1, cv_accuracy, plus tol, and the refit
             at the best C per slice in svms/svm_b{block}_t{t1}.npz (evaluate.py:364-413)

Transfer (`-d/--data {cifar10, tiny-imagenet-200}`, evaluate.py:30, 38-51, 311-312, 368-371): `features RUN -d NAME --data-file F.pt`
extracts the features of ANOTHER dataset's test images (`x_test` uint8 [N, C, H, W], `y_test` in F.pt) with the run's net:
resized to the side the run was trained on (`train.SHAPES`) exactly as `transforms.Resize` does on a PIL image, and normalised
with the RUN dataset's statistics -- always, whatever the run's `--augmentation` was -- in one HIP launch per chunk
(`augment.TransferTransform`) -> features-NAME.npz; `retrieval -d NAME` and `finetune -d NAME` read that file and write
retrieval-NAME.csv, finetune-NAME.csv and svms-NAME/.  (The reference writes the transfer SVMs over the run's own `svms/`;
that quirk is not kept.)  NAME only names the files: the images are the file's.

A run trained with `train --model resnet` (the baseline, resnet.py) takes `features` -- seven "time points": the stem's output and
the outputs of the six blocks, `t1s = linspace(0, 1, 7)`, `tols = [0]` (evaluate.py:65-67) -- and `retrieval` and `finetune` on them; the
modes that sweep the ODE block (`nfe`, `tradeoff`, `accuracy`) refuse it.

Runs on a run directory written by `neural_ode_features_amd.train` (or any `{'params', 'model'}` checkpoint with the
reference's state_dict keys).  Test data: `--data file.pt` (`x_test`, `y_test`) or the synthetic set of that run; a run
trained with `--augmentation` gets its test transform (augment.py), a run without the key is taken as `none`.

    python -m neural_ode_features_amd.evaluate features runs_cifar10/odenet --t1 0 0.5 1 --tol 1e-3 1e-1
    python -m neural_ode_features_amd.evaluate nfe runs_cifar10/odenet --limit 100
    python -m neural_ode_features_amd.evaluate retrieval runs_cifar10/odenet
    python -m neural_ode_features_amd.evaluate finetune runs_cifar10/odenet --aggregate
    python -m neural_ode_features_amd.evaluate features runs_cifar10/odenet -d tiny-imagenet-200 --data-file tiny_val.pt
    python -m neural_ode_features_amd.evaluate finetune runs_cifar10/odenet -d tiny-imagenet-200
"""
from __future__ import annotations

import argparse
import itertools
import os
import sys
import types

import numpy as np
import torch


TRANSFER_DATA = ('cifar10', 'tiny-imagenet-200')          # evaluate.py:448, 451, 457
TRANSFER_CHUNK = 1024                                     # images per launch of the transfer transform


def result_name(name, data):
    """`features.npz` -> `features-<data>.npz` with `-d <data>` (evaluate.py:30, 311-312, 368-370); the same for directories."""
    if data is None:
        return name
    stem, ext = os.path.splitext(name)
    return '%s-%s%s' % (stem, data, ext)


def load_transfer_file(path, in_ch):
    """(`x_test` uint8 [N, in_ch, H, W], `y_test` [N]) of a `--data-file`, or a SystemExit that says what is wrong with it."""
    if not os.path.exists(path):
        raise SystemExit('--data-file %s not found' % path)
    blob = torch.load(path, map_location='cpu')
    if not isinstance(blob, dict) or 'x_test' not in blob or 'y_test' not in blob:
        raise SystemExit('--data-file %s must hold x_test (uint8 [N, C, H, W]) and y_test' % path)
    x, y = blob['x_test'], blob['y_test']
    if not torch.is_tensor(x) or x.dtype != torch.uint8 or x.dim() != 4:
        raise SystemExit('--data-file %s: x_test must be a uint8 tensor [N, C, H, W] (the resize starts from the 8-bit pixels); it is %s'
                         % (path, '%s %s' % (x.dtype, tuple(x.shape)) if torch.is_tensor(x) else type(x).__name__))
    if x.shape[1] != in_ch:
        raise SystemExit('--data-file %s holds %d-channel images, the run was trained on %d-channel images'
                         % (path, x.shape[1], in_ch))
    if not torch.is_tensor(y) or y.dim() != 1 or y.shape[0] != x.shape[0]:
        raise SystemExit('--data-file %s: y_test must hold one label per image of x_test' % path)
    return x, y


def transfer_test_set(p, data_file, device):
    """evaluate.py:38-51: the file's test images resized to the side the run was trained on and normalised with the run
    dataset's statistics, on the device, in chunks -> (fp32 [N, C, side, side] on the device, labels on the host)."""
    import neural_ode_features_amd as nof
    from .train import SHAPES
    in_ch, side, _ = SHAPES[p.dataset]
    x, y = load_transfer_file(data_file, in_ch)
    split = nof.DeviceSplit(x, y, device)
    tt = nof.TransferTransform(side, dataset=p.dataset)
    order = torch.arange(len(split), device=split.device)
    return torch.cat([tt.batch(split, order[i:i + TRANSFER_CHUNK])[0] for i in range(0, len(split), TRANSFER_CHUNK)]), y.cpu()


def load_run(run_dir, which='best'):
    """`utils.load_model` stand-in (utils.py:248-270): rebuild the net from the run's params, load its weights."""
    import neural_ode_features_amd as nof
    path = os.path.join(run_dir, which + '.pth')
    if not os.path.exists(path):
        path = os.path.join(run_dir, 'last.pth')
    ckpt = torch.load(path, map_location='cpu', weights_only=False)
    p = types.SimpleNamespace(**ckpt['params'])
    from .resnet import build_model
    from .train import SHAPES, load_data
    if getattr(p, 'data', None):
        blob = torch.load(p.data, map_location='cpu')
        xte, yte = blob['x_test'], blob['y_test']
        in_ch, out = xte.shape[1], int(blob['y_train'].max()) + 1
    else:
        _, _, xte, yte, in_ch, out = load_data(p)
    kind = getattr(p, 'augmentation', 'none')        # a run of before the flag has no such key
    if kind != 'none':
        # an augmented run trained on the device pipeline's images: the test set goes through its test transform (ToTensor,
        # plus Normalize for the `...+norm` kinds) and stays on the device
        if not torch.cuda.is_available():
            raise SystemExit('neural_ode_features_amd.evaluate needs a HIP device: the input pipeline has no CPU path')
        if xte.dtype != torch.uint8:
            raise SystemExit('the run was trained with --augmentation %s: its test images must be uint8 (they are %s)' % (kind, xte.dtype))
        aug = nof.Augmenter(kind, dataset=p.dataset, seed=p.seed)
        split = nof.DeviceSplit(xte, yte, torch.device('cuda'))
        order = torch.arange(len(split), device=split.device)
        xte = torch.cat([aug.batch(split, order[i:i + 1024], 0, train=False)[0] for i in range(0, len(split), 1024)])
    model = build_model(p, in_ch, out)           # a ResNet for `params.model == 'resnet'`; no such key: an ODENet
    model.load_state_dict(ckpt['model'])
    return model, p, xte, yte


def _is_resnet(p):
    return getattr(p, 'model', 'odenet') == 'resnet'


def _needs_odenet(p, mode):
    if _is_resnet(p):
        raise SystemExit('evaluate %s sweeps the ODE block\'s tolerance and integration time: the run is a ResNet, which has no '
                         'ODE block (its modes: features, retrieval, finetune)' % mode)


def features(args):
    """evaluate.py:24-94."""
    model, p, xte, yte = load_run(args.run)
    data = getattr(args, 'data', None)
    if data is not None:                              # evaluate.py:38-51: another dataset's test images through the run's net
        xte, yte = transfer_test_set(p, args.data_file, args.device)
    if args.limit:
        xte, yte = xte[:args.limit], yte[:args.limit]
    model = model.to(args.device).eval()
    model.to_features_extractor()
    resnet = _is_resnet(p)
    if resnet:       # evaluate.py:65-67: seven "time points" (the stem's output and the six blocks'), no tolerance
        args.t1, args.tol = np.linspace(0, 1, 7).tolist(), [0]
    else:
        model.odeblock.t1 = list(args.t1)
        if 'ode' in p.downsample:
            model.downsample.odeblock.t1 = list(args.t1)
    feats = []
    with torch.no_grad():
        for tol in args.tol:
            if not resnet:
                model.odeblock.tol = tol
            f = [model(xte[i:i + p.batch_size].to(args.device)).cpu().numpy() for i in range(0, xte.shape[0], p.batch_size)]
            feats.append(np.concatenate(f, -2))       # concat along the batch dimension
    out = os.path.join(args.run, result_name('features.npz', data))
    np.savez(out, features=np.stack(feats), y_true=yte.numpy(), tols=np.array(args.tol), t1s=np.array(args.t1))
    print('features', np.stack(feats).shape, '->', out)
    return out


def nfe(args):
    """evaluate.py:97-142: per-image function evaluations, batch size 1."""
    import pandas as pd
    model, p, xte, yte = load_run(args.run)
    _needs_odenet(p, 'nfe')
    if args.limit:
        xte, yte = xte[:args.limit], yte[:args.limit]
    model = model.to(args.device).eval()
    rows = []
    with torch.no_grad():
        for tol, t1 in itertools.product(args.tol, args.t1):
            # (t1 = 0 is the identity block, model.py:363-364: rows with nfe = 0, as the reference writes them)
            model.odeblock.t1 = t1
            model.odeblock.tol = tol
            model.nfe(reset=True)
            for i in range(xte.shape[0]):
                pred = model(xte[i:i + 1].to(args.device)).argmax(dim=1).item()
                rows.append({'y_true': int(yte[i]), 'y_pred': pred, 'nfe': model.nfe(reset=True), 't1': t1, 'tol': tol})
    out = os.path.join(args.run, 'nfe.csv.gz')
    df = pd.DataFrame(rows)
    df.to_csv(out, index=False)
    print(df.groupby(['tol', 't1']).nfe.mean())
    return out


def _test_batches(xte, yte, bs, device):
    for i in range(0, xte.shape[0], bs):
        yield xte[i:i + bs].to(device), yte[i:i + bs].to(device)


def tradeoff(args):
    """evaluate.py:145-204: accuracy / NFE trade-off over `tol x t1`, the live block mutated between forwards."""
    import pandas as pd
    import torch.nn.functional as F
    model, p, xte, yte = load_run(args.run)
    _needs_odenet(p, 'tradeoff')
    if args.limit:
        xte, yte = xte[:args.limit], yte[:args.limit]
    model = model.to(args.device).eval()
    rows = []
    with torch.no_grad():
        for tol, t1 in itertools.product(args.tol, args.t1):
            model.odeblock.t1 = t1
            model.odeblock.tol = tol
            model.nfe(reset=True)
            n_correct = n_processed = n_batches = nfe_forward = 0
            loss = None
            for x, y in _test_batches(xte, yte, p.batch_size, args.device):
                pr = model(x)
                nfe_forward += model.nfe(reset=True)
                loss = F.cross_entropy(pr, y)
                n_correct += int((y == pr.argmax(dim=1)).sum())
                n_processed += y.shape[0]
                n_batches += 1
            # (the reference reports the LAST batch's mean loss over the images processed so far, evaluate.py:181: kept as it is)
            rows.append({'t1': t1, 'test_loss': float(loss) / n_processed, 'test_acc': n_correct / n_processed,
                         'test_nfe': nfe_forward / n_batches, 'test_tol': tol})
    out = os.path.join(args.run, 'tradeoff.csv')
    df = pd.DataFrame(rows)
    df.to_csv(out, index=False)
    print(df)
    return out


def accuracy(args):
    """evaluate.py:207-305: the classifier's loss / accuracy at every time slice of ONE dense-output solve per batch."""
    import pandas as pd
    import torch.nn.functional as F
    from .head import trajectory_loss
    from .odenet import FCClassifier
    model, p, xte, yte = load_run(args.run)
    _needs_odenet(p, 'accuracy')
    if args.limit:
        xte, yte = xte[:args.limit], yte[:args.limit]
    model = model.to(args.device).eval()
    t1 = torch.arange(0, 1.05, .05) if args.t1 is None or len(args.t1) < 2 else torch.tensor([0.0] + [t for t in args.t1 if t > 0])
    model.odeblock.t1 = t1[1:].tolist()           # 0 is implicit (evaluate.py:231)
    model.odeblock.return_last_only = False
    if p.downsample == 'ode2':
        model.downsample.odeblock.t1 = t1[1:].tolist()
        model.downsample.odeblock.return_last_only = False
        model.downsample.odeblock.apply_conv = True
        t1 = torch.cat((t1, t1))
    T = len(t1)
    frames = []
    with torch.no_grad():
        for tol in args.tol:
            model.odeblock.tol = tol
            if 'ode' in p.downsample:
                model.downsample.odeblock.tol = tol
            model.nfe(reset=True)
            n_correct, tot_losses = torch.zeros(T), torch.zeros(T)
            n_processed = n_batches = nfe_forward = 0
            for x, y in _test_batches(xte, yte, p.batch_size, args.device):
                pr = model(x)                                      # timestamps (T) x batch (N) x classes (C)
                nfe_forward += model.nfe(reset=True)
                if FCClassifier.fused_trajectory:
                    # every slice's summed loss and hit count: one launch and one read-back (head.trajectory_loss)
                    stat = trajectory_loss(pr, y).cpu()
                    tot_losses += stat[:, 0]
                    n_correct += stat[:, 1]
                else:       # the ATen chain, as before that kernel existed (A/B runs, tests)
                    losses = F.cross_entropy(pr.permute(1, 2, 0), y.unsqueeze(1).expand(-1, T), reduction='none')      # N x T
                    tot_losses += losses.sum(0).cpu()
                    n_correct += (y.unsqueeze(0).expand(T, -1) == pr.argmax(dim=-1)).sum(-1).float().cpu()
                n_processed += y.shape[0]
                n_batches += 1
            frames.append(pd.DataFrame({'t1': t1.numpy(), 'test_loss': (tot_losses / n_processed).numpy(),
                                        'test_acc': (n_correct / n_processed).numpy(), 'test_nfe': [nfe_forward / n_batches] * T,
                                        'test_tol': [tol] * T}))
    out = os.path.join(args.run, 'results')
    df = pd.concat(frames, ignore_index=True)
    df.to_csv(out, index=False)
    print(df)
    return out


def retrieval(args, k=10):
    """evaluate.py:308-361: per-query AP and AP@10 of the test set against itself, features of every time slice as queries,
    on the HIP kernels of `retrieval.average_precision` instead of one sklearn call per query.

    The reference's `features()` writes `[tols, T, N, D]` while its `retrieval()` indexes `[T, N, D]`, so the reference loop
    runs here once per tolerance slice.  Everything else is kept as written, quirks included: the features are normalised
    along axis -2 (the SAMPLE axis, not the feature axis) plus 1e-7, on the host in numpy, so that the scores start from
    bit-for-bit the reference's inputs; 'asym' ranks the database of the last time slice, 'sym' that of the query's own
    slice (for 'ode' stems, whose slices are 2T, the same indices); every image is a query, and the query itself stays in
    the database.  -> retrieval.csv with the reference's columns ap_asym, ap_sym, ap10_asym, ap10_sym, t1, plus tol: one
    row per (tol, t1, query).  With `-d NAME`: features-NAME.npz -> retrieval-NAME.csv."""
    import pandas as pd
    from .retrieval import average_precision
    data = getattr(args, 'data', None)
    path = os.path.join(args.run, result_name('features.npz', data))
    if not os.path.exists(path):
        raise SystemExit('no pre-extracted features found: %s (run the `features` mode first)' % path)
    with np.load(path) as f:
        feats, y_true, t1s, tols = f['features'], f['y_true'], f['t1s'], f['tols']
    feats = feats / (np.linalg.norm(feats, axis=-2, keepdims=True) + 1e-7)
    labels = torch.from_numpy(y_true.astype(np.int32)).to(args.device)
    frames = []
    for ti, tol in enumerate(tols):
        fd = torch.from_numpy(np.ascontiguousarray(feats[ti])).to(args.device)          # [T, N, D]
        for i, t1 in enumerate(t1s):
            ap_asym, ap10_asym = average_precision(fd[i], fd[-1], labels, labels, k=k)   # t1 = 1 for the database
            ap_sym, ap10_sym = average_precision(fd[i], fd[i], labels, labels, k=k)      # the same t1 for queries and database
            frames.append(pd.DataFrame({'ap_asym': ap_asym.cpu().numpy(), 'ap_sym': ap_sym.cpu().numpy(),
                                        'ap10_asym': ap10_asym.cpu().numpy(), 'ap10_sym': ap10_sym.cpu().numpy(),
                                        't1': t1, 'tol': tol}))
    out = os.path.join(args.run, result_name('retrieval.csv', data))
    df = pd.concat(frames, ignore_index=True)
    df.to_csv(out, index=False)
    print(df.groupby(['tol', 't1']).mean())
    return out


def _run_params(run_dir, which='best'):
    """The `params` of the run's checkpoint alone (no model, no data)."""
    path = os.path.join(run_dir, which + '.pth')
    if not os.path.exists(path):
        path = os.path.join(run_dir, 'last.pth')
    if not os.path.exists(path):
        raise SystemExit('no checkpoint found in %s (best.pth / last.pth)' % run_dir)
    return types.SimpleNamespace(**torch.load(path, map_location='cpu', weights_only=False)['params'])


def _svc_search(feats, y_true):
    """One slice's grid search on the device: `finetune.linear_svc_cv` on features [N, D] (numpy) and labels."""
    from .finetune import linear_svc_cv
    if not torch.cuda.is_available():
        raise SystemExit('neural_ode_features_amd.evaluate needs a HIP device: the SVM solver has no CPU path')
    dev = torch.device('cuda')
    x = torch.from_numpy(np.ascontiguousarray(feats, dtype=np.float32)).to(dev)
    return linear_svc_cv(x, torch.from_numpy(np.asarray(y_true).astype(np.int64)).to(dev))


def finetune(args):
    """evaluate.py:364-413: the 5-fold cross-validated accuracy of a linear SVM (C searched over logspace(-2, 2, 5)) on the
    features of every time slice, as one batch of problems per slice on the HIP solver of `finetune.linear_svc_cv` instead of
    sklearn's GridSearchCV on the host.

    The reference's `features()` writes `[tols, T, N, D]` while its `finetune()` indexes `[T, N, D]`, so the reference loop runs
    here once per tolerance slice.  Kept as written: `--aggregate` replaces the slices by their mean over T with `t1 = -1`;
    for `downsample == 'ode'` runs the slices are those of the ODE stem then those of the ODE block, `block = [0] * T + [1] * T`
    with `t1s` doubled; slices, `t1s` and `block` are zipped.  -> finetune.csv with the reference's columns block, t1,
    cv_accuracy, plus tol: one row per (tol, slice); the refit at the best C (the reference pickles the estimator) as `coef
    [K, D]`, `intercept [K]`, `C` and `classes` in svms/svm_b{block}_t{t1}.npz, with `_tol{tol}` before the suffix when the
    features hold more than one tolerance.  With `-d NAME`: features-NAME.npz -> finetune-NAME.csv and svms-NAME/ (the reference
    writes these SVMs into the run's own `svms/`, over those of the run's dataset: not kept)."""
    import pandas as pd
    data = getattr(args, 'data', None)
    path = os.path.join(args.run, result_name('features.npz', data))
    if not os.path.exists(path):
        raise SystemExit('no pre-extracted features found: %s (run the `features` mode first)' % path)
    p = _run_params(args.run)
    with np.load(path) as f:
        feats, y_true, t1s, tols = f['features'], f['y_true'], f['t1s'], f['tols']
    svm_dir = os.path.join(args.run, result_name('svms', data))
    os.makedirs(svm_dir, exist_ok=True)
    rows = []
    for ti, tol in enumerate(tols):
        fs, ts = feats[ti], t1s                                                          # [T, N, D]
        if getattr(args, 'aggregate', False):
            fs, ts = fs.mean(0, keepdims=True), np.array([-1])
        block = np.zeros(len(ts), dtype=int)
        if getattr(p, 'downsample', None) == 'ode':
            block, ts = np.concatenate((block, block + 1)), np.concatenate((ts, ts))
        for t1, b, fi in zip(ts, block, fs):
            search = _svc_search(fi, y_true)
            rows.append({'block': int(b), 't1': t1, 'cv_accuracy': search.best_score, 'tol': tol})
            name = 'svm_b%d_t%g%s.npz' % (b, t1, '_tol%g' % tol if len(tols) > 1 else '')
            np.savez(os.path.join(svm_dir, name), coef=search.coef, intercept=search.intercept, C=search.best_C,
                     classes=search.classes)
    out = os.path.join(args.run, result_name('finetune.csv', data))
    df = pd.DataFrame(rows, columns=['block', 't1', 'cv_accuracy', 'tol'])
    df.to_csv(out, index=False)
    print(df)
    return out


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description='features / nfe / tradeoff / accuracy / retrieval / finetune evaluations of the reference on the HIP '
                                             'backend')
    ap.add_argument('mode', choices=('features', 'nfe', 'tradeoff', 'accuracy', 'retrieval', 'finetune'))
    ap.add_argument('run')
    ap.add_argument('--t1', type=float, nargs='+', default=np.arange(0, 1.05, .05).tolist())      # evaluate.py:424
    ap.add_argument('--tol', type=float, nargs='+', default=[1e-3, 1e-2, 1e-1, 1e0, 1e1, 1e2])      # evaluate.py:423
    ap.add_argument('--limit', type=int, default=0, help='only the first N test images')
    ap.add_argument('-a', '--aggregate', action='store_true', help='finetune: one slice, the mean of the features over t1')
    ap.add_argument('-d', '--data', choices=TRANSFER_DATA, default=None,
                    help='features / retrieval / finetune: the transfer variant -- features of --data-file through the run\'s net, '
                         'in files named after it')
    ap.add_argument('--data-file', default=None, help='features -d: a .pt with x_test (uint8 [N, C, H, W]) and y_test')
    args = ap.parse_args(argv)
    if args.data is not None and args.mode not in ('features', 'retrieval', 'finetune'):
        raise SystemExit('-d/--data is a switch of features, retrieval and finetune (evaluate.py:448-457), not of %s' % args.mode)
    if args.data_file is not None and (args.data is None or args.mode != 'features'):
        raise SystemExit('--data-file goes with `features -d/--data NAME`')
    if args.mode == 'features' and args.data is not None and args.data_file is None:
        raise SystemExit('features -d %s needs --data-file FILE.pt (x_test uint8 [N, C, H, W], y_test): datasets are files here'
                         % args.data)
    return args


def main(argv=None):
    args = parse_args(argv)
    if args.mode == 'finetune':          # reads files only; the solver asks for the device when the first slice reaches it
        return finetune(args)
    if not torch.cuda.is_available():
        raise SystemExit('neural_ode_features_amd.evaluate needs a HIP device: the ODE block has no CPU path')
    args.device = torch.device('cuda')
    return {'features': features, 'nfe': nfe, 'tradeoff': tradeoff, 'accuracy': accuracy, 'retrieval': retrieval}[args.mode](args)


if __name__ == '__main__':
    main()

#!/usr/bin/env python
"""Cost of the transfer transform (augment.TransferTransform.batch, csrc/kernels_resize.hip) on a test set of 10 000 colour
images, for the reference's two pairings (32 -> 64 and 64 -> 32), next to what the same work costs without it.

    python3 tools/resize_time.py [--out profiles/resize_time.txt] [--images 10000] [--repeats 10]

fused   ONE launch for the whole set: gather, PIL-exact resize, ToTensor, Normalize.  HIP events around the call (the
        allocation of the output from torch's cache + the launch), operands cache-cold: between two timed calls a 1 GiB
        buffer is rewritten, four times the 256 MiB Infinity Cache.
        Reported with the bytes the launch must move (uint8 pixels in, fp32 out, index and labels) over that time.
host    what a user had to do before: `Image.resize` per image with Pillow on 16 host processes, one upload of the resized
        uint8 set, then `Augmenter.batch(train=False)` in chunks of 1024 (ToTensor + Normalize on the device).  Wall time
        per stage; the Pillow stage runs first, before this process touches the GPU (the workers never do).  Without Pillow
        the stage is reported as not measured.

Both paths produce the same fp32 tensor, bit for bit; the tool checks that before it reports."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PAIRS = ((32, 64, 'tiny-imagenet-200'), (64, 32, 'cifar10'))          # (side in, side out, the statistics of the run's dataset)
WORKERS = 16


def _images(n, side, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (n, 3, side, side), dtype=np.uint8), rng.integers(0, 10, n).astype(np.int64)


def _pil_chunk(job):
    from PIL import Image
    x, side = job
    out = np.empty((x.shape[0], 3, side, side), dtype=np.uint8)
    for i, img in enumerate(x):
        rgb = Image.fromarray(np.ascontiguousarray(img.transpose(1, 2, 0)), 'RGB').resize((side, side), Image.BILINEAR)
        out[i] = np.asarray(rgb).transpose(2, 0, 1)
    return out


def pil_stage(sets, repeats):
    """{side in: (resized uint8 set, [seconds per repeat])}, or None without Pillow.  Runs before the GPU is initialised."""
    try:
        import PIL  # noqa: F401
    except ImportError:
        return None
    import multiprocessing as mp
    out = {}
    with mp.get_context('fork').Pool(WORKERS) as pool:
        for side_in, side_out, _ in PAIRS:
            x = sets[side_in][0]
            jobs = [(c, side_out) for c in np.array_split(x, WORKERS * 4)]
            pool.map(_pil_chunk, jobs[:WORKERS])                       # warm-up: imports in the workers
            times = []
            for _ in range(repeats):
                t0 = time.perf_counter()
                res = np.concatenate(pool.map(_pil_chunk, jobs))
                times.append(time.perf_counter() - t0)
            out[side_in] = (res, times)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join('profiles', 'resize_time.txt'))
    ap.add_argument('--images', type=int, default=10000)
    ap.add_argument('--repeats', type=int, default=10)
    args = ap.parse_args()
    n = args.images
    sets = {side_in: _images(n, side_in, side_in) for side_in, _, _ in PAIRS}
    host = pil_stage(sets, 3)

    import torch
    import neural_ode_features_amd as nof
    if not torch.cuda.is_available():
        raise SystemExit('tools/resize_time.py needs a HIP device: a time measured anywhere else says nothing')
    lines = ['transfer transform on %d images of 3 channels, %s' % (n, torch.cuda.get_device_name(0))]
    flush = torch.empty(1 << 30, dtype=torch.uint8, device='cuda')
    for side_in, side_out, dataset in PAIRS:
        x, y = sets[side_in]
        split = nof.DeviceSplit(torch.from_numpy(x), torch.from_numpy(y), 'cuda')
        order = torch.arange(n, device='cuda')
        tt = nof.TransferTransform(side_out, dataset=dataset)
        moved = n * (3 * side_in * side_in + 4 * 3 * side_out * side_out + 8 + 8 + 8)
        for _ in range(2):                                             # warm-up: the tables, the code object, torch's cache
            images, _ = tt.batch(split, order)
        torch.cuda.synchronize()
        times = []
        for _ in range(args.repeats):
            del images
            flush.add_(1)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            images, _ = tt.batch(split, order)
            b.record()
            b.synchronize()
            times.append(a.elapsed_time(b) * 1e3)
        t = np.array(times)
        lines.append('%d -> %d  fused  TransferTransform.batch, one launch, cache-cold, HIP events around the call: median %.1f us  '
                     'min %.1f  max %.1f  (%d calls);  %.1f MB to move -> %.0f GB/s at the median'
                     % (side_in, side_out, np.median(t), t.min(), t.max(), len(t), moved / 1e6, moved / np.median(t) / 1e3))
        if host is None:
            lines.append('%d -> %d  host   Pillow is not installed here: not measured' % (side_in, side_out))
            continue
        resized, pil_times = host[side_in]
        aug = nof.Augmenter('crop+flip+norm', dataset=dataset)
        up, dev = [], []
        for _ in range(4):                                             # the first: warm-up
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rsplit = nof.DeviceSplit(torch.from_numpy(resized), torch.from_numpy(y), 'cuda')
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            ref = torch.cat([aug.batch(rsplit, order[i:i + 1024], 0, train=False)[0] for i in range(0, n, 1024)])
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            up.append(t1 - t0)
            dev.append(t2 - t1)
        if not torch.equal(ref, images):
            raise SystemExit('%d -> %d: the fused launch and Pillow + Augmenter.batch differ' % (side_in, side_out))
        pil, upl, tr = np.median(pil_times) * 1e3, np.median(up[1:]) * 1e3, np.median(dev[1:]) * 1e3
        lines.append('%d -> %d  host   Pillow resize on %d processes %.1f ms + upload %.2f ms + Augmenter.batch(train=False) in chunks of '
                     '1024 %.2f ms = %.1f ms (medians of 3 wall times each; the same tensor, bit for bit) -> %.0f x the fused launch'
                     % (side_in, side_out, WORKERS, pil, upl, tr, pil + upl + tr, (pil + upl + tr) * 1e3 / np.median(t)))
        del ref, rsplit
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()

"""Writes tests/golden/resize_pil.npz: what Pillow's `Image.resize((out_w, out_h), Image.BILINEAR)` returns on 8-bit images,
the reference of csrc/kernels_resize.hip (the reference's `transforms.Resize` on a PIL image, evaluate.py:38-50).

    python tests/golden/make_golden_resize.py

Per size pair k: `in_k` uint8 [3, C, H, W] -- image 0 random pixels, image 1 all 255, image 2 a 0 / 255 checkerboard (shifted by
one per channel) -- and `out_k` uint8 [3, C, OH, OW], each channel resized as an 'L' image (what PIL does with the bands of an
RGB image); `cases` int64 [K, 5] holds (C, H, W, OH, OW).  Needs Pillow; the tests that read the file do not."""
import os

import numpy as np
from PIL import Image

# (C, H, W, OH, OW): the reference's two pairings, MNIST to 64, the identity, two rectangles, a strong reduction (9 taps and
# more per output), a strong enlargement, and a reduction by a non-integer factor on both axes
CASES = [(3, 32, 32, 64, 64), (3, 64, 64, 32, 32), (1, 28, 28, 64, 64), (3, 32, 32, 32, 32), (3, 20, 36, 9, 50),
         (3, 64, 64, 7, 7), (3, 5, 5, 64, 64), (3, 64, 64, 48, 40)]


def images(c, h, w, seed):
    rng = np.random.default_rng(seed)
    ch, row, col = np.meshgrid(np.arange(c), np.arange(h), np.arange(w), indexing='ij')
    return np.stack([rng.integers(0, 256, (c, h, w), dtype=np.uint8), np.full((c, h, w), 255, np.uint8),
                     (((ch + row + col) % 2) * 255).astype(np.uint8)])


def pil_resize(x, oh, ow):
    """x uint8 [..., H, W] -> [..., OH, OW], plane by plane."""
    flat = x.reshape((-1,) + x.shape[-2:])
    out = np.stack([np.asarray(Image.fromarray(p, 'L').resize((ow, oh), Image.BILINEAR)) for p in flat])
    return out.reshape(x.shape[:-2] + (oh, ow))


def main():
    blob = {'cases': np.array(CASES, dtype=np.int64)}
    for k, (c, h, w, oh, ow) in enumerate(CASES):
        x = images(c, h, w, 1000 + k)
        blob['in_%d' % k] = x
        blob['out_%d' % k] = pil_resize(x, oh, ow)
    # an RGB image is resized band by band: the plane-by-plane form above is what `Resize` does to a colour image
    x = blob['in_0'][0]
    rgb = np.asarray(Image.fromarray(np.ascontiguousarray(x.transpose(1, 2, 0)), 'RGB').resize((64, 64), Image.BILINEAR))
    assert np.array_equal(rgb.transpose(2, 0, 1), blob['out_0'][0])
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'resize_pil.npz')
    np.savez_compressed(path, **blob)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()

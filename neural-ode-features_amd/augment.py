"""The reference's training augmentations (`--augmentation`, utils.py:81-196) on the HIP backend: the split lives on the
device as uint8, and ONE launch per batch (csrc/kernels_augment.hip) turns a batch of dataset indices into the network's
input -- gather, RandomCrop with zero padding, ColorJitter(saturation, hue), RandomHorizontalFlip, ToTensor, Normalize --
plus the gathered labels.  No host-to-device copy and no synchronisation per batch.

    split = DeviceSplit(x_uint8, y, device)                        # [N, C, H, W] uint8, [N] labels: uploaded once
    aug = Augmenter('crop+jitter+flip+norm', dataset='cifar10', seed=23)
    images, target = aug.batch(split, index, epoch)                # index: int64 device tensor of dataset indices
    images, target = aug.batch(split, index, 0, train=False)       # the test transform: ToTensor (+ Normalize)

The random numbers are Philox4x32-10 keyed by `seed` and counted by (dataset index, epoch): an image's augmentation does not
depend on the batch it arrives in, its position there, the batch size or the rank, and a batch that is run a second time
(`integrate.DeferredLoop` after a missed step count) sees the same pixels.  The jitter follows torchvision's tensor
formulas in fp32, not PIL's 8-bit HSV path.  There is no CPU path.

The transfer evaluations' test transform (evaluate.py:38-50 of the reference: `Resize(side)`, `ToTensor`, `Normalize` on a PIL
image) is one launch per batch as well (csrc/kernels_resize.hip): PIL's 8-bit bilinear resample, bit for bit.

    tt = TransferTransform(64, dataset='tiny-imagenet-200')        # a CIFAR-10 split for a net trained on 64-pixel images
    images, target = tt.batch(split, index)                        # fp32 [B, C, 64, 64], normalised
    pixels = tt.resized(split, index)                              # uint8 [B, C, 64, 64]: what PIL's resize returns
"""
from __future__ import annotations

import torch

from . import _lib

KINDS = ('none', 'crop', 'crop+flip+norm', 'crop+jitter+flip+norm')
FLAGS = {
    'none': 0,
    'crop': _lib.AUG_CROP,
    'crop+flip+norm': _lib.AUG_CROP | _lib.AUG_FLIP | _lib.AUG_NORM,
    'crop+jitter+flip+norm': _lib.AUG_CROP | _lib.AUG_JITTER | _lib.AUG_FLIP | _lib.AUG_NORM,
}
# utils.py:13-19
PREPROC = {
    'mnist': ((0.0,), (1.0,)),
    'cifar10': ((0.4914, 0.4822, 0.4465), (0.2023, 0.1994, 0.2010)),
    'cifar100': ((0.5071, 0.4865, 0.4409), (0.2673, 0.2564, 0.2762)),
    'tiny-imagenet-200': ((0.4802, 0.4481, 0.3975), (0.2770, 0.2691, 0.2821)),
}
SATURATION = HUE = 0.05                                  # ColorJitter(hue=.05, saturation=.05), utils.py:117
PADDING = {28: 4, 32: 4, 64: 8}                          # RandomCrop(size, padding), by image side (utils.py:87,103,173)


class DeviceSplit:
    """One split of a dataset in device memory: images uint8 [N, C, H, W] (C 1 or 3), labels int64 [N]."""

    def __init__(self, x_uint8, y, device):
        if not torch.is_tensor(x_uint8) or x_uint8.dim() != 4:
            raise ValueError('images must be a 4-D tensor [N, C, H, W]')
        if x_uint8.dtype != torch.uint8:
            raise TypeError('images must be uint8 (got %s): the device pipeline starts from the 8-bit pixels' % x_uint8.dtype)
        if x_uint8.shape[0] < 1 or x_uint8.shape[1] not in (1, 3):
            raise ValueError('images must be [N >= 1, C in (1, 3), H, W] (got %s)' % (tuple(x_uint8.shape),))
        if not torch.is_tensor(y) or y.dim() != 1 or y.shape[0] != x_uint8.shape[0]:
            raise ValueError('labels must be a 1-D tensor of %d entries' % x_uint8.shape[0])
        if y.dtype.is_floating_point or y.dtype.is_complex or y.dtype == torch.bool:
            raise TypeError('labels must be integers (got %s)' % y.dtype)
        device = torch.device(device)
        if device.type != 'cuda':
            raise RuntimeError('augment has no CPU path: a split must live on a HIP device (got %s)' % device)
        self.x = x_uint8.to(device).contiguous()
        self.y = y.to(device=device, dtype=torch.int64).contiguous()
        self.device = self.x.device

    def __len__(self):
        return self.x.shape[0]


class Augmenter:
    """The transform chain `kind` of the reference.  `dataset` picks Normalize's statistics (PREPROC) unless `mean` / `std`
    are given; `padding` defaults to the reference's for the image side (4 for 28 and 32 pixels, 8 for 64)."""

    def __init__(self, kind, dataset=None, mean=None, std=None, padding=None, seed=0):
        if kind not in KINDS:
            raise ValueError('augmentation %r: one of %s' % (kind, ', '.join(KINDS)))
        self.kind, self.flags = kind, FLAGS[kind]
        if (mean is None) != (std is None):
            raise ValueError('mean and std come together')
        if mean is None and self.flags & _lib.AUG_NORM:
            if dataset not in PREPROC:
                raise ValueError('%r needs the statistics of a known dataset (%s) or mean= and std=' % (kind, ', '.join(PREPROC)))
            mean, std = PREPROC[dataset]
        self.mean = tuple(float(m) for m in mean) if mean is not None else None
        self.std = tuple(float(s) for s in std) if std is not None else None
        if self.std is not None and (len(self.std) != len(self.mean) or len(self.std) not in (1, 3) or min(self.std) <= 0):
            raise ValueError('mean and std must hold 1 or 3 entries each, std > 0')
        if padding is not None and (isinstance(padding, bool) or int(padding) != padding or not 0 <= padding < 32768):
            raise ValueError('padding must be an integer in [0, 32768) (got %r)' % (padding,))
        self.padding = None if padding is None else int(padding)
        self.saturation, self.hue = SATURATION, HUE
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF

    def padding_for(self, h, w):
        if self.padding is not None:
            return self.padding
        if h != w or h not in PADDING:
            raise ValueError('no reference padding for %d x %d images: pass padding=' % (h, w))
        return PADDING[h]

    def descriptor(self, split_shape, train=True):
        """The node_augment record of this chain on a split of shape [N, C, H, W]."""
        n, c, h, w = (int(v) for v in split_shape)
        flags = self.flags if train else self.flags & _lib.AUG_NORM
        if flags & _lib.AUG_JITTER and c != 3:
            raise ValueError('colour jitter needs 3 channels (got %d)' % c)
        d = _lib.NodeAugment(n, c, h, w, self.padding_for(h, w) if flags & _lib.AUG_CROP else 0, flags, self.saturation, self.hue)
        if flags & _lib.AUG_NORM:
            if len(self.mean) != c:
                raise ValueError('%d-channel statistics for %d-channel images' % (len(self.mean), c))
            d.mean[:c], d.std[:c] = self.mean, self.std
        return d

    def batch(self, split, index, epoch, train=True):
        """(images fp32 [B, C, H, W], target int64 [B]) of the dataset indices `index` (int64, on the split's device), enqueued
        on the current stream.  `train=False`: the test transform -- ToTensor, plus Normalize for the `...+norm` kinds."""
        if not isinstance(split, DeviceSplit):
            raise TypeError('split must be a DeviceSplit')
        if not torch.is_tensor(index) or index.dim() != 1 or index.dtype != torch.int64:
            raise TypeError('index must be a 1-D int64 tensor')
        if not index.is_cuda:
            raise RuntimeError('augment has no CPU path: index must live on a HIP device (got %s)' % index.device)
        if index.device != split.device:
            raise RuntimeError('index must live on %s (got %s)' % (split.device, index.device))
        if isinstance(epoch, bool) or int(epoch) != epoch or not 0 <= epoch < 1 << 32:
            raise ValueError('epoch must be an integer in [0, 2^32) (got %r)' % (epoch,))
        desc = self.descriptor(split.x.shape, train)
        index = index.contiguous()
        b = index.shape[0]
        images = torch.empty((b,) + tuple(split.x.shape[1:]), dtype=torch.float32, device=split.device)
        target = torch.empty(b, dtype=torch.int64, device=split.device)
        if b == 0:
            return images, target
        lib = _lib.load()
        with torch.cuda.device(split.device):
            _lib.check(lib.node_augment_batch(desc, split.x.data_ptr(), split.y.data_ptr(), index.data_ptr(), b, self.seed,
                                              int(epoch), images.data_ptr(), target.data_ptr(),
                                              torch.cuda.current_stream(split.device).cuda_stream))
        return images, target


class TransferTransform:
    """`Resize(size)`, `ToTensor` and -- with `dataset` (PREPROC) or `mean` / `std` -- `Normalize`, as the reference applies them
    to another dataset's test images (evaluate.py:38-50).  `size` is the output side, or `(h, w)`; the resize is PIL's
    `Image.resize((w, h), Image.BILINEAR)` on the 8-bit image, bit for bit, and a size the split already has is the identity.
    (torchvision's `Resize(int)` scales the SHORTER side and keeps the aspect ratio: the same thing on the square images of
    the reference's datasets, and only there.)"""

    def __init__(self, size, dataset=None, mean=None, std=None):
        if isinstance(size, (tuple, list)):
            if len(size) != 2:
                raise ValueError('size must be an integer or (h, w) (got %r)' % (size,))
            h, w = size
        else:
            h = w = size
        for v in (h, w):
            if isinstance(v, bool) or not isinstance(v, int) or v < 1:
                raise ValueError('size must be an integer >= 1 or a pair (h, w) of them (got %r)' % (size,))
        self.size = (h, w)
        if (mean is None) != (std is None):
            raise ValueError('mean and std come together')
        if mean is None and dataset is not None:
            if dataset not in PREPROC:
                raise ValueError('%r is not a known dataset (%s): pass mean= and std=' % (dataset, ', '.join(PREPROC)))
            mean, std = PREPROC[dataset]
        self.mean = tuple(float(m) for m in mean) if mean is not None else None
        self.std = tuple(float(s) for s in std) if std is not None else None
        if self.std is not None and (len(self.std) != len(self.mean) or len(self.std) not in (1, 3) or min(self.std) <= 0):
            raise ValueError('mean and std must hold 1 or 3 entries each, std > 0')

    def descriptor(self, split_shape):
        """The node_resize record of this transform on a split of shape [N, C, H, W]."""
        n, c, h, w = (int(v) for v in split_shape)
        d = _lib.NodeResize(n, c, h, w, self.size[0], self.size[1], int(self.mean is not None))
        if self.mean is not None:
            if len(self.mean) != c:
                raise ValueError('%d-channel statistics for %d-channel images' % (len(self.mean), c))
            d.mean[:c], d.std[:c] = self.mean, self.std
        return d

    def _launch(self, split, index, want_f32):
        if not isinstance(split, DeviceSplit):
            raise TypeError('split must be a DeviceSplit')
        if not torch.is_tensor(index) or index.dim() != 1 or index.dtype != torch.int64:
            raise TypeError('index must be a 1-D int64 tensor')
        if not index.is_cuda:
            raise RuntimeError('augment has no CPU path: index must live on a HIP device (got %s)' % index.device)
        if index.device != split.device:
            raise RuntimeError('index must live on %s (got %s)' % (split.device, index.device))
        desc = self.descriptor(split.x.shape)
        index = index.contiguous()
        b = index.shape[0]
        images = torch.empty((b, split.x.shape[1]) + self.size, dtype=torch.float32 if want_f32 else torch.uint8, device=split.device)
        target = torch.empty(b, dtype=torch.int64, device=split.device)
        if b == 0:
            return images, target
        lib = _lib.load()
        with torch.cuda.device(split.device):
            _lib.check(lib.node_resize_batch(desc, split.x.data_ptr(), split.y.data_ptr(), index.data_ptr(), b,
                                             images.data_ptr() if want_f32 else None, None if want_f32 else images.data_ptr(),
                                             target.data_ptr(), torch.cuda.current_stream(split.device).cuda_stream))
        return images, target

    def batch(self, split, index):
        """(images fp32 [B, C, h, w], target int64 [B]) of the dataset indices `index` (int64, on the split's device), enqueued
        on the current stream: resized, / 255, normalised when the transform has statistics."""
        return self._launch(split, index, True)

    def resized(self, split, index):
        """The resized 8-bit images alone, uint8 [B, C, h, w]: what `ToTensor` is applied to."""
        return self._launch(split, index, False)[0]

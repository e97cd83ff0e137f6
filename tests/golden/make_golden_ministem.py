"""Generate the reference fixture of the `minimal` stem.

Run in the build container only (it imports the reference's ``model.py`` unchanged, the way make_golden.py does), on the CPU:

    python tests/golden/make_golden_ministem.py

  stem_minimal_c64.pt   reference ``MinimalConvDownsample(1, 64)`` (model.py:129-145: Conv2d(1, 24, 3, 1), two
                        GroupNorm(24, 24) + ReLU, two 4x4 stride-2 convolutions) on a [2, 1, 28, 28] input: input, cotangent,
                        output, state_dict and every parameter gradient

Fixtures are data (tensors).  No reference source text is stored.
"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import import_reference_model  # noqa: E402


def make_ministem(ref):
    torch.manual_seed(61)
    gen = torch.Generator().manual_seed(61)
    stem = ref.MinimalConvDownsample(1, out_ch=64)
    with torch.no_grad():       # (the Sequential's GroupNorms are `module.1`, `module.4`)
        for i in (1, 4):
            stem.module[i].weight.copy_(1.0 + 0.25 * torch.randn(24, generator=gen))
            stem.module[i].bias.copy_(0.1 * torch.randn(24, generator=gen))
    x = torch.rand(2, 1, 28, 28, generator=gen)
    out = stem(x)
    cot = torch.randn(out.shape, generator=gen)
    out.backward(cot)
    torch.save({'x': x, 'cot': cot, 'out': out.detach(), 'state_dict': stem.state_dict(),
                'grads': {k: v.grad.clone() for k, v in stem.named_parameters()}},
               os.path.join(HERE, 'stem_minimal_c64.pt'))
    print('stem_minimal_c64: out %s, %d parameter tensors' % (tuple(out.shape), len(list(stem.parameters()))))


if __name__ == '__main__':
    make_ministem(import_reference_model())

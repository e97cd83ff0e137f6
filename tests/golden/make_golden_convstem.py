"""Generate the reference fixtures of the `convolution` stem and of the `ode2` stem's hand-off.

Run in the build container only (it imports the reference's ``model.py`` unchanged, the way make_golden.py does):

    python tests/golden/make_golden_convstem.py

  stem_convolution_c64.pt   reference ``ConvDownsample(1, 64)`` (model.py:148-164: Conv2d(1, 64, 3, 1), two GroupNorm + ReLU,
                            two 4x4 stride-2 convolutions) on a [2, 1, 28, 28] input: output, cotangent and state_dict;
  stem_convolution_c64_grads.pt   every parameter gradient of that run (a file of its own: each stays under 1 MiB)
  ode2_handoff_c64.pt       reference ``ODEDownsample2(1, 64)`` (model.py:199-223): its own ``.norm`` and ``.conv2`` --
                            ``conv2(norm(x))``, what sits between the stem's two solves -- on a [2, 64, 14, 14] input:
                            output, cotangent, the two modules' state_dicts, the input gradient and the four parameter gradients

Fixtures are data (tensors).  No reference source text is stored.
"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import import_reference_model, randomize_  # noqa: E402


def make_convstem(ref):
    torch.manual_seed(53)
    gen = torch.Generator().manual_seed(53)
    stem = ref.ConvDownsample(1, out_ch=64)
    with torch.no_grad():       # (the Sequential's GroupNorms are `module.1`, `module.4`: no 'norm' in their names)
        for i in (1, 4):
            stem.module[i].weight.copy_(1.0 + 0.25 * torch.randn(64, generator=gen))
            stem.module[i].bias.copy_(0.1 * torch.randn(64, generator=gen))
    x = torch.rand(2, 1, 28, 28, generator=gen)
    out = stem(x)
    cot = torch.randn(out.shape, generator=gen)
    out.backward(cot)
    # two files: the two 64 x 64 x 4 x 4 filters and their gradients are 0.5 MB each way, and no stored vector exceeds 1 MiB
    torch.save({'x': x, 'cot': cot, 'out': out.detach(), 'state_dict': stem.state_dict()},
               os.path.join(HERE, 'stem_convolution_c64.pt'))
    torch.save({'grads': {k: v.grad.clone() for k, v in stem.named_parameters()}},
               os.path.join(HERE, 'stem_convolution_c64_grads.pt'))
    print('stem_convolution_c64: out %s, %d parameter tensors' % (tuple(out.shape), len(list(stem.parameters()))))


def make_handoff(ref):
    torch.manual_seed(59)
    gen = torch.Generator().manual_seed(59)
    stem = ref.ODEDownsample2(1, out_ch=64)
    randomize_(stem, gen)
    x = torch.randn(2, 64, 14, 14, generator=gen).requires_grad_(True)
    out = stem.conv2(stem.norm(x.clone()))      # (the ReLU is in place: keep the leaf's values)
    cot = torch.randn(out.shape, generator=gen)
    out.backward(cot)
    torch.save({'x': x.detach(), 'cot': cot, 'out': out.detach(), 'd_x': x.grad.clone(),
                'norm': stem.norm.state_dict(), 'conv2': stem.conv2.state_dict(),
                'grads': {'norm.0.weight': stem.norm[0].weight.grad.clone(), 'norm.0.bias': stem.norm[0].bias.grad.clone(),
                          'conv2.weight': stem.conv2.weight.grad.clone(), 'conv2.bias': stem.conv2.bias.grad.clone()}},
               os.path.join(HERE, 'ode2_handoff_c64.pt'))
    print('ode2_handoff_c64: out %s' % (tuple(out.shape),))


if __name__ == '__main__':
    ref_model = import_reference_model()
    make_convstem(ref_model)
    make_handoff(ref_model)

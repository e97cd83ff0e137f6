#!/usr/bin/env python
"""Generate the ResNet-baseline fixtures under tests/golden/ from the REFERENCE itself (its `model.py`, imported
unchanged through `make_golden.import_reference_model`; needs the reference checkout, which never travels):

    python tests/golden/make_golden_resnet.py

  resnet_keys.json        state_dict keys and shapes, in order, of the reference's `ResNet(3, n_filters=256,
                          downsample='residual')` and `ResNet(1, n_filters=64, downsample='one-shot')` (model.py:65-111)
  resnet_oneshot_c16.pt   the reference's `ResNet(1, out=10, n_filters=16, downsample='one-shot')` on x [3, 1, 28, 28]: the
                          state_dict, eval logits, cross-entropy loss and every parameter gradient in train mode, the
                          [7, 3, 16] output after `to_features_extractor()` and, on a fresh copy, the shape of the output after
                          `to_features_extractor(keep_pool=False)`
  resnet_trunk2_c64.pt    the reference's `nn.Sequential(ResBlock(64, 64), ResBlock(64, 64))` (model.py:284-310) on
                          x [2, 64, 7, 7], GroupNorm weights and biases perturbed by 0.2 randn, a random cotangent: the
                          state_dict, the output, the input gradient and every parameter gradient.  The four filters are
                          rounded to values a bfloat16 holds exactly and stored in that type (half the bytes, nothing lost:
                          `load_state_dict` widens them back to the very fp32 numbers the reference computed with), which
                          keeps the file under 1 MiB; everything else is fp32.

Fixtures are data (tensors / json).  No reference source text is stored.
"""
import copy
import json
import os
import sys

import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import import_reference_model  # noqa: E402


def perturb_norms_(module, gen):
    with torch.no_grad():
        for name, p in module.named_parameters():
            if 'norm' in name:
                p.add_(0.2 * torch.randn(p.shape, generator=gen))


def make_keys(ref):
    out = {}
    for tag, net in (('resnet_3_f256_residual', ref.ResNet(3, n_filters=256, downsample='residual')),
                     ('resnet_1_f64_one-shot', ref.ResNet(1, n_filters=64, downsample='one-shot'))):
        out[tag] = [[k, list(v.shape)] for k, v in net.state_dict().items()]
    with open(os.path.join(HERE, 'resnet_keys.json'), 'w') as fh:
        json.dump(out, fh, indent=0)
    print('resnet_keys:', {k: len(v) for k, v in out.items()})


def make_oneshot_c16(ref):
    torch.manual_seed(71)
    gen = torch.Generator().manual_seed(72)
    net = ref.ResNet(1, out=10, n_filters=16, downsample='one-shot')
    perturb_norms_(net, gen)
    x = torch.randn(3, 1, 28, 28, generator=gen)
    y = torch.tensor([3, 0, 7])
    state = {k: v.clone() for k, v in net.state_dict().items()}
    net.eval()
    with torch.no_grad():
        logits = net(x)
    net.train()
    loss = F.cross_entropy(net(x), y)
    loss.backward()
    grads = {k: p.grad.clone() for k, p in net.named_parameters()}
    pooled = copy.deepcopy(net).eval()
    pooled.to_features_extractor()
    with torch.no_grad():
        feats = pooled(x)
    unpooled = copy.deepcopy(net).eval()
    unpooled.to_features_extractor(keep_pool=False)
    with torch.no_grad():
        full = unpooled(x)
    assert tuple(feats.shape) == (7, 3, 16), feats.shape
    torch.save({'x': x, 'y': y, 'state_dict': state, 'logits': logits, 'loss': loss.detach(), 'grads': grads, 'features': feats,
                'features_nopool_shape': list(full.shape)}, os.path.join(HERE, 'resnet_oneshot_c16.pt'))
    print('resnet_oneshot_c16: logits %s, features %s, without pool %s' % (tuple(logits.shape), tuple(feats.shape), tuple(full.shape)))


def make_trunk2_c64(ref):
    torch.manual_seed(73)
    gen = torch.Generator().manual_seed(74)
    trunk = torch.nn.Sequential(ref.ResBlock(64, 64), ref.ResBlock(64, 64))
    perturb_norms_(trunk, gen)
    with torch.no_grad():
        for name, p in trunk.named_parameters():
            if 'conv' in name:
                p.copy_(p.bfloat16().float())
    x = torch.randn(2, 64, 7, 7, generator=gen).requires_grad_(True)
    out = trunk(x)
    cot = torch.randn(out.shape, generator=gen)
    out.backward(cot)
    state = {k: (v.bfloat16() if 'conv' in k else v.clone()) for k, v in trunk.state_dict().items()}
    for k, v in trunk.state_dict().items():
        assert torch.equal(state[k].float(), v), k
    path = os.path.join(HERE, 'resnet_trunk2_c64.pt')
    torch.save({'x': x.detach(), 'cot': cot, 'out': out.detach(), 'dx': x.grad.clone(), 'state_dict': state,
                'grads': {k: p.grad.clone() for k, p in trunk.named_parameters()}}, path)
    print('resnet_trunk2_c64: out %s, %d bytes' % (tuple(out.shape), os.path.getsize(path)))
    assert os.path.getsize(path) < (1 << 20)


if __name__ == '__main__':
    ref = import_reference_model()
    make_keys(ref)
    make_oneshot_c16(ref)
    make_trunk2_c64(ref)

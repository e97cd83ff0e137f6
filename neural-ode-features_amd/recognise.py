"""Recognising the reference's conv `ODEfunc` (`model.py:326-348`): the ten parameters and the GroupNorm configuration
the fused kernels take, duck-typed, and remembered per function object."""
from __future__ import annotations

import weakref
from typing import List

import torch
from torch import nn

PARAM_ATTRS = [
    ('norm1', 'weight'), ('norm1', 'bias'), ('conv1', 'weight'), ('conv1', 'bias'),
    ('norm2', 'weight'), ('norm2', 'bias'), ('conv2', 'weight'), ('conv2', 'bias'),
    ('norm3', 'weight'), ('norm3', 'bias'),
]


class Recognised:
    """The ten parameters + GroupNorm config of a conv ODEfunc (duck-typed so the
    reference's own `model.ODEfunc` instance is accepted unchanged)."""

    def __init__(self, func: nn.Module):
        def conv_of(m):
            layer = getattr(m, '_layer', None)
            if not isinstance(layer, nn.Conv2d):
                raise NotImplementedError('ConcatConv2d with a plain nn.Conv2d `_layer` expected')
            if layer.kernel_size != (3, 3) or layer.stride != (1, 1) or layer.padding != (1, 1) \
                    or layer.dilation != (1, 1) or layer.groups != 1 or layer.bias is None:
                raise NotImplementedError('only Conv2d(dim+1, dim, 3, 1, 1, bias=True) dynamics are accelerated')
            return layer

        for name in ('norm1', 'conv1', 'norm2', 'conv2', 'norm3'):
            if not hasattr(func, name):
                raise NotImplementedError(
                    'neural-ode-features_amd accelerates the reference ODEfunc (model.py:326-348) only; '
                    '%s has no attribute %r' % (type(func).__name__, name))
        norms = [func.norm1, func.norm2, func.norm3]
        for nrm in norms:
            if not isinstance(nrm, nn.GroupNorm):
                raise NotImplementedError("only norm='group' dynamics are accelerated (BatchNorm couples samples)")
            if not nrm.affine:
                raise NotImplementedError('GroupNorm must be affine')
        c1, c2 = conv_of(func.conv1), conv_of(func.conv2)
        dim = norms[0].num_channels
        for nrm in norms:
            if nrm.num_channels != dim or nrm.num_groups != norms[0].num_groups or nrm.eps != norms[0].eps:
                raise NotImplementedError('the three GroupNorms must share channels / groups / eps')
        for cv in (c1, c2):
            if cv.in_channels != dim + 1 or cv.out_channels != dim:
                raise NotImplementedError('ConcatConv2d(dim, dim) expected')
        self.dim, self.groups, self.eps = dim, norms[0].num_groups, float(norms[0].eps)
        self.params: List[torch.Tensor] = [
            func.norm1.weight, func.norm1.bias, c1.weight, c1.bias,
            func.norm2.weight, func.norm2.bias, c2.weight, c2.bias,
            func.norm3.weight, func.norm3.bias]
        # must equal func.parameters() order: defines the flat-gradient layout
        own = list(func.parameters())
        if len(own) != 10 or any(a is not b for a, b in zip(own, self.params)):
            raise NotImplementedError('ODEfunc.parameters() is not the expected ten tensors in reference order')


# Recognised(func) walks the module tree (named_modules, parameters): ~25 us per call, once per solve.  The result is remembered per
# func OBJECT (weakly) together with the identities it was built from -- the five sub-modules, the two conv layers, the ten parameter
# objects, the counts of func's own entries -- and rebuilt when any of them is another object (a replaced layer or parameter, a
# `load_state_dict` keeps the objects and needs nothing).
_REC_SEEN: "weakref.WeakKeyDictionary" = weakref.WeakKeyDictionary()


def _rec_signature(func):
    try:      # (straight through the modules' own dicts: nn.Module.__getattr__ costs ~0.4 us per lookup, this runs once per solve)
        m = func._modules
        n1, c1, n2, c2, n3 = m['norm1'], m['conv1'], m['norm2'], m['conv2'], m['norm3']
        l1, l2 = c1._modules['_layer'], c2._modules['_layer']
        p1, q1, p2, q2, p3 = n1._parameters, l1._parameters, n2._parameters, l2._parameters, n3._parameters
        return (id(n1), id(c1), id(n2), id(c2), id(n3), id(l1), id(l2),
                id(p1['weight']), id(p1['bias']), id(q1['weight']), id(q1['bias']), id(p2['weight']), id(p2['bias']),
                id(q2['weight']), id(q2['bias']), id(p3['weight']), id(p3['bias']), n1.num_groups, n1.eps, len(m), len(func._parameters))
    except (AttributeError, KeyError):
        return None


def recognised(func: nn.Module) -> Recognised:
    """Recognised(func), remembered per object; raises NotImplementedError like the constructor."""
    sig = _rec_signature(func)
    if sig is not None:
        try:
            hit = _REC_SEEN.get(func)
        except TypeError:       # (an unhashable / non-weakly-referenceable object: no cache)
            hit, sig = None, None
        if hit is not None and hit[0] == sig:
            return hit[1]
    rec = Recognised(func)
    if sig is not None:
        _REC_SEEN[func] = (sig, rec)
    return rec

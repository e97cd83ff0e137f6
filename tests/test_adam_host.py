"""CPU-side checks of the fused Adam step: the C layout of its table record against the ctypes mirror, and what
optim.FusedAdam does without touching a device -- torch.optim.Adam's parameter-group keys, the scheduler surface, and the
refusals (unsupported modes first, then the CPU)."""
import ctypes as C
import os
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_adam_tensor_layout_matches_the_ctypes_mirror(tmp_path):
    """include/node_hip.h still compiles as pedantic C99 with the new record in it, and node_adam_tensor has the size and
    the field offsets the C compiler gives it (the method of test_header_is_plain_c_and_ctypes_layouts_match)."""
    from neural_ode_features_amd import _lib
    fields = ['param', 'grad', 'exp_avg', 'exp_avg_sq', 'step', 'n']
    assert [f for f, _ in _lib.NodeAdamTensor._fields_] == fields
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "node_hip.h"', 'int main(void) {',
             '  printf("size %zu\\n", sizeof(node_adam_tensor));']
    lines += ['  printf("%s %%zu\\n", offsetof(node_adam_tensor, %s));' % (f, f) for f in fields]
    lines += ['  return 0;', '}']
    src = tmp_path / 'adam_abi.c'
    src.write_text('\n'.join(lines))
    exe = tmp_path / 'adam_abi'
    subprocess.check_call(['gcc', '-std=c99', '-Wall', '-Werror', '-pedantic', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got['size']) == C.sizeof(_lib.NodeAdamTensor)
    for f in fields:
        assert int(got[f]) == getattr(_lib.NodeAdamTensor, f).offset, f
    assert 'node_adam_step' in _lib.EXPORTS and hasattr(_lib.load(), 'node_adam_step')


def _stepped_once():
    import neural_ode_features_amd as nof
    lin = torch.nn.Linear(3, 2)
    opt = nof.FusedAdam(lin.parameters(), lr=1e-3, weight_decay=1e-4)
    lin(torch.ones(1, 3)).sum().backward()
    return lin, opt


def test_fused_adam_refuses_the_cpu():
    _, opt = _stepped_once()
    with pytest.raises(RuntimeError, match='no CPU path'):
        opt.step()


def test_fused_adam_has_torch_adams_param_group_keys_and_takes_schedulers():
    import neural_ode_features_amd as nof
    lin, opt = _stepped_once()
    ref = torch.optim.Adam(lin.parameters(), lr=1e-3, weight_decay=1e-4)
    mine, theirs = opt.state_dict()['param_groups'][0], ref.state_dict()['param_groups'][0]
    assert set(mine) == set(theirs)
    assert set(mine) == {'params', 'lr', 'betas', 'eps', 'weight_decay', 'amsgrad', 'maximize', 'foreach', 'capturable',
                         'differentiable', 'fused', 'decoupled_weight_decay'}
    assert mine == theirs                                   # the defaults are torch.optim.Adam's, value for value
    assert isinstance(opt, torch.optim.Optimizer) and nof.FusedAdam is nof.optim.FusedAdam
    # the reference's three schedules (train.py:158-163) attach and drive param_groups
    torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda=lambda x: 1)
    torch.optim.lr_scheduler.ReduceLROnPlateau(opt, mode='max', patience=10)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, 4)
    assert opt.param_groups[0]['initial_lr'] == 1e-3 and sched.get_last_lr() == [1e-3]
    # a parameter-group dictionary of torch.optim.Adam loads, and the reverse
    opt.load_state_dict(ref.state_dict())
    ref.load_state_dict(opt.state_dict())
    # FusedSGD keeps the surface it had beside the shared base
    sgd = nof.FusedSGD(lin.parameters(), lr=0.1, momentum=0.9)
    assert sgd.grad_scale == 1.0 and sgd.skip_flag is None and sgd.flags_to_reset == []
    assert set(sgd.state_dict()['param_groups'][0]) == set(torch.optim.SGD(lin.parameters(), lr=0.1).state_dict()['param_groups'][0])


@pytest.mark.parametrize('mode', ['amsgrad', 'maximize', 'decoupled_weight_decay'])
def test_fused_adam_refuses_unsupported_modes_before_it_looks_at_the_device(mode):
    _, opt = _stepped_once()                                # CPU parameters: the mode is refused first
    opt.param_groups[0][mode] = True
    with pytest.raises(ValueError, match=mode):
        opt.step()
    opt.param_groups[0][mode] = False
    with pytest.raises(RuntimeError, match='no CPU path'):
        opt.step()
    import neural_ode_features_amd as nof
    for bad in (dict(lr=-1.0), dict(eps=-1e-8), dict(weight_decay=-0.1), dict(betas=(1.0, 0.999)), dict(betas=(0.9, -0.1))):
        with pytest.raises(ValueError):
            nof.FusedAdam([torch.zeros(2, requires_grad=True)], **bad)

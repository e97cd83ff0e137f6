"""neural-ode-features_amd -- MI355X-native drop-in for the ODE-block hot path of
fabiocarrara/neural-ode-features.

Aliasable as `torchdiffeq` (it exports `odeint` and `odeint_adjoint`), so the
reference's `model.py` runs unchanged on top of the HIP library:

    import neural_ode_features_amd, sys
    sys.modules['torchdiffeq'] = neural_ode_features_amd      # before `import model`
"""
from .integrate import odeint, odeint_adjoint, odefunc_forward, odefunc_vjp  # noqa: F401
from .modules import ConcatConv2d, ODEBlock, ODEfunc, normalization  # noqa: F401
from .odenet import FCClassifier, ODEDownsample, ODEDownsample2, ODENet, ResBlock, StackedODENet  # noqa: F401
from . import attack, augment, bnsolve, dp, finetune, graphs, optim, retrieval  # noqa: F401
from .augment import Augmenter, DeviceSplit, TransferTransform  # noqa: F401
from .imgconv import ImageConv2d  # noqa: F401
from .convstem import ConvStem  # noqa: F401
from .ministem import MinimalStem  # noqa: F401
from .downconv import bn_relu_conv, gn_relu_conv  # noqa: F401
from .pool import max_pool_4s2, trajectory_pool  # noqa: F401
from .resnet import ResNet, ResidualTrunk, build_model  # noqa: F401
from .optim import FusedAdam, FusedSGD  # noqa: F401
from .head import cross_entropy, linear, linear_cross_entropy, trajectory_distance, trajectory_loss  # noqa: F401

__all__ = ['odeint', 'odeint_adjoint', 'ODEBlock', 'ODEfunc', 'ConcatConv2d', 'ODENet', 'StackedODENet', 'ResNet', 'ResidualTrunk',
           'ODEDownsample', 'ODEDownsample2', 'ConvStem', 'MinimalStem', 'max_pool_4s2', 'trajectory_pool', 'dp']

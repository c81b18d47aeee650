"""stribor_amd — MI355X-native drop-in for stribor's coupling-flow hot path.

Same names and constructor signatures as ``stribor`` for the classes on the path
(``NormalizingFlow``, ``Coupling``, ``Affine``, ``Spline``, ``AffineLU``, ``MatrixExponential``,
``Permute``/``Flip``, ``Sigmoid``/``Logit``, ``ELU``, ``LeakyReLU``, ``ContinuousTanh``, ``ContinuousActivation``, ``Cumsum``/``Diff``,
``CumsumColumn``/``DiffColumn``, ``Identity``,
``IResNet``/``ContinuousIResNet``, ``ContinuousTransform`` (with ``net.DiffeqMLP``, ``net.DiffeqDeepset``, ``net.DiffeqExactTraceMLP``,
``net.DiffeqExactTraceDeepSet``), ``UnitNormal``, ``Normal``, ``MultivariateNormal``, ``Uniform``, ``UnitUniform``, ``net.MLP``, ``net.ResNet``/``net.ResNetBlock``, ``net.attention``/``net.Attention``/``net.SelfAttention``/
``net.InducedSelfAttention``, ``util.get_mask``, ``util.safe_softmax``); the arithmetic is hand-written
HIP for gfx950 behind the C ABI in ``include/stribor_hip.h``.  There is no CPU fallback.
"""
from . import net, util
from . import dist
from .dist import *          # noqa: F401,F403
from .dist.normal import UnitNormal
from .densities import MultivariateNormal, Normal, Uniform, UnitUniform, log_prob_closed_form
from .flow import ElementwiseTransform, NeuralFlow, NormalizingFlow, Transform
from .flows import (ELU, Affine, AffineLU, ContinuousActivation, ContinuousAffineCoupling, ContinuousIResNet, ContinuousTanh, ContinuousTransform, Coupling,
                    Cumsum, CumsumColumn, Diff, DiffColumn, Flip, Identity, IResNet, LeakyReLU, Logit, MatrixExponential, Permute, Sigmoid, Spline)

from ._hip import GemmRangeError, check_errors, get_gemm_precision, set_gemm_precision, set_sync_errors

__version__ = '0.2.0'

# the reference's `stribor.dist` namespace: the densities with parameters live in densities.py and are exported from there as well
for _name in ('Normal', 'MultivariateNormal', 'Uniform', 'UnitUniform', 'log_prob_closed_form'):
    setattr(dist, _name, globals()[_name])
del _name

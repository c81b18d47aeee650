from .affine import Affine
from .coupling import ContinuousAffineCoupling, Coupling
from .permute import Flip, Permute
from .spline import Spline
from .linear import AffineLU, MatrixExponential
from .pointwise import ELU, Cumsum, CumsumColumn, Diff, DiffColumn, Identity, LeakyReLU, Logit, Sigmoid
from .time_pointwise import ContinuousActivation, ContinuousTanh
from .iresnet import ContinuousIResNet, IResNet
from .cnf import ContinuousTransform

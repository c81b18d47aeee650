from .mlp import MLP
from .resnet import ResNet, ResNetBlock
from .time_net import TimeFourier, TimeFourierBounded, TimeIdentity, TimeLinear, TimeLog, TimeTanh
from .attention import Attention, InducedSelfAttention, SelfAttention, attention, self_attention_closed_form
from .equivariant import EquivariantLayer, EquivariantNet, equivariant_backward_closed_form
from .diffeq import DiffeqConcat, DiffeqDeepset, DiffeqMLP, DiffeqNet, DiffeqSelfAttention
from .made import MADE
from .diffeq_zero_trace import DiffeqZeroTraceDeepSet, DiffeqZeroTraceMLP
from .diagjac import FuncAndDiagJac
from .diffeq_exact_trace import DiffeqExactTrace, DiffeqExactTraceDeepSet, DiffeqExactTraceMLP

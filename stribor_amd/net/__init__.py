from .mlp import MLP
from .time_net import TimeFourier, TimeFourierBounded, TimeIdentity, TimeLinear, TimeLog, TimeTanh
from .attention import Attention, InducedSelfAttention, SelfAttention, attention
from .diffeq import DiffeqConcat, DiffeqMLP, DiffeqNet

from .conv_variational import *
from .linear_variational import *
from .local_reparam import *
from .rnn_variational import *
from .quantized_variational import *

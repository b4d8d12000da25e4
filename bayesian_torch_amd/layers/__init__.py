"""bayesian_torch_amd.layers — same export surface as the reference `bayesian_torch/layers/__init__.py:1-6`
(the variational-forward hot path, the LSTM wrappers over its Linear layers and the INT8 twins of Linear / Conv2d Reparameterization
and Linear / Conv2d Flipout: no quantized LSTM and, of the tuple-passing wrappers, `Dropout` only — SURVEY.md §2 scope), plus the
Monte-Carlo dropout layers MCDropout / MCDropout1d/2d/3d (dropout_layers.py)."""
from . import variational_layers
from . import flipout_layers
from .variational_layers import *
from .flipout_layers import *
from .base_variational_layer import BaseVariationalLayer_, get_kernel_size, set_backend
from . import dropout_layers
from .dropout_layers import MCDropout, MCDropout1d, MCDropout2d, MCDropout3d, Dropout  # BTX-DROP v1

from .dnn_to_bnn import dnn_to_bnn, get_kl_loss  # noqa: F401
from .fuse import fuse_model  # noqa: F401
from .bnn_to_qbnn import bnn_to_qbnn  # noqa: F401

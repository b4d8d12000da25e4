from .dnn_to_bnn import dnn_to_bnn, get_kl_loss, set_prior  # noqa: F401
from .fuse import fuse_model  # noqa: F401
from .bnn_to_qbnn import bnn_to_qbnn  # noqa: F401
from .mc_dropout import enable_mc_dropout  # noqa: F401
from .qresnet import QBasicBlock, QBottleneck, QResNet, to_qresnet, qresnet18, qresnet34, qresnet50, qresnet101  # noqa: F401

from .util import get_rho, entropy, predictive_entropy, mutual_information  # noqa: F401
from . import avuc_loss, uncertainty_calibration_loss  # noqa: F401
from . import mc_loss  # noqa: F401
from .mc_loss import MCCrossEntropy, MCGaussianNLL, mc_elbo_loss, mc_gaussian_nll  # noqa: F401
from .checkpoint import checkpoint  # noqa: F401  (utils.checkpoint is the FUNCTION from here on: it shadows the submodule of that name)

from .util import get_rho, entropy, predictive_entropy, mutual_information  # noqa: F401
from . import avuc_loss, uncertainty_calibration_loss  # noqa: F401

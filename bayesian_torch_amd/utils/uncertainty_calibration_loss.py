"""utils.uncertainty_calibration_loss — EaU / EaC (regression) and AvU (classification) calibration losses (reference
utils/uncertainty_calibration_loss.py; https://arxiv.org/abs/2012.07923,
https://link.springer.com/chapter/10.1007/978-3-031-25072-9_31).  Each forward returns a 0-d tensor.

Dispatch is that of utils.avuc_loss: CPU tensors and set_backend("torch") run the vectorised ATen chain; 1-D f32 CUDA
error / unc / conf run libbtx.so (btx_eau_fwd / btx_eau_bwd), CUDA logits run btx_avu_fwd / btx_avu_bwd.  Thresholds are Python
numbers or 0-d / 1-element tensors on the inputs' device (read by the kernel when it runs).

Deviation from the reference: inputs are flattened to 1-D and the real value is computed.  For column vectors [B, 1] — and for
B == 1 in its AvULoss — the reference returns the degenerate -beta * log(1e-10), because every torch.dot falls into its `except`.
"""
from torch import nn

from . import _calibration as _c


class EaULoss(nn.Module):
    """Error aligned Uncertainty: good = error <= error_th, certain = unc <= unc_th,
    weights (1 - tanh error | tanh error) x (1 - tanh unc | tanh unc)"""

    def __init__(self, beta=1):
        super().__init__()
        self.beta = beta
        self.eps = _c.EPS

    def forward(self, error, unc, error_th, unc_th):
        return _c.eau(error, unc, error_th, unc_th, self.beta, False)


class EaCLoss(nn.Module):
    """Error aligned Confidence: good = error <= error_th, certain = conf > conf_th,
    weights (1 - tanh error | tanh error) x (conf | 1 - conf)"""

    def __init__(self, beta=1):
        super().__init__()
        self.beta = beta
        self.eps = _c.EPS

    def forward(self, error, conf, error_th, conf_th):
        return _c.eau(error, conf, error_th, conf_th, self.beta, True)


class AvULoss(nn.Module):
    """Accuracy versus Uncertainty at one threshold on the predictive entropy of logits [B, C]"""

    def __init__(self, beta=1):
        super().__init__()
        self.beta = beta
        self.eps = _c.EPS

    def forward(self, logits, labels, unc_th):
        return _c.avu(logits, labels, unc_th, self.beta, False)[0].reshape(())

"""utils.avuc_loss — Accuracy versus Uncertainty Calibration losses (reference utils/avuc_loss.py; Krishnan & Tickoo, NeurIPS
2020, https://arxiv.org/abs/2012.07923), vectorised, and on the GPU fused into three HIP launches without a host read.

    avu = AvULoss(beta=3.0)
    loss = ce(out, y) + kl / bs + avu(out, y, threshold)        # works inside autograd.GraphedTrainStep(loss_fn=...)

CPU tensors and set_backend("torch") run the vectorised ATen chain of utils/_calibration.py; CUDA logits [B, C] in f32 or bf16
with int64 labels and C <= mc.MC_MAX_CLASSES run libbtx.so (btx_avu_fwd / btx_avu_bwd, loss in f32, dlogits in the logits'
dtype); other GPU inputs run the chain on the device.  The threshold may be a Python number (baked in) or a 0-d / 1-element
tensor on the logits' device, which the kernel reads when it runs: a captured graph follows a per-epoch threshold update.

Deviations from the reference:
  * reference AUAvULoss.forward does not run (sklearn's auc on tensors that require grad; torch.log of a float without); this
    module implements its evident intent — AvU at the 21 thresholds, trapezoid over np.linspace(0, 1, 21), loss =
    -beta * log(auc + 1e-10) — differentiably.  The value oracle is the reference's own auc_avu() helper.
  * thresholds th_k = umin + t_k (umax - umin) are evaluated in double from the f32 umin / umax and compared with the entropy
    promoted to double; th_20 = umax exactly.  The reference rounds umax - umin in f32 first, which makes the membership of the
    most uncertain example at t = 1 a last-bit coin flip.
  * type=1 (model uncertainty) takes MC-stacked [S, B, C] logits (autograd.mc_train_forward, or the `out` of
    GraphedTrainStep(num_mc=S)) and labels [B]: p_s = softmax(logits_s), pbar = mean_s p_s, confidence / prediction from pbar, the
    uncertainty is the mutual information H(pbar) - mean_s H(p_s) (epsilon 1e-10 inside every log), then the same quadrant
    arithmetic; gradients flow through the soft weights into all S samples.  CUDA stacks with S <= 32 and C <= 16128 run btx_avu_mc_fwd / _bwd,
    everything else the chain.  The reference gives no oracle value here: its forward applies softmax(dim=1) to whatever it gets,
    i.e. over the BATCH axis of a stack.  On 2-D logits type=1 raises ValueError (the reference indexes a 0-d tensor and crashes);
    3-D logits with type=0 raise as well.
  * the arg-max tie-break is the lowest index; no print of the counts.
"""
import numpy as np
import torch
from torch import nn

from . import _calibration as _c


def _avu(logits, labels, th, beta, area, type):
    if type == 0:
        return _c.avu(logits, labels, th, beta, area)
    if type == 1:
        return _c.avu_mc(logits, labels, th, beta, area)
    raise ValueError("type must be 0 (predictive entropy, [batch, classes] logits) or 1 (model uncertainty, Monte-Carlo stacked "
                     "[S, batch, classes] logits), got %r" % (type,))


class AvULoss(nn.Module):
    """loss [1] = -beta * log(AvU + 1e-10) of logits [B, C] (type=0) or an MC stack [S, B, C] (type=1) and labels [B] at one
    uncertainty threshold"""

    def __init__(self, beta=1):
        super().__init__()
        self.beta = beta
        self.eps = _c.EPS

    def forward(self, logits, labels, optimal_uncertainty_threshold, type=0):
        return _avu(logits, labels, optimal_uncertainty_threshold, self.beta, False, type)[0]


class AUAvULoss(nn.Module):
    """(loss [1], auc_avu [1]): the area under AvU over 21 thresholds between the least and the most uncertain example of the
    batch, no threshold to choose.  Both outputs carry gradient."""

    def __init__(self, beta=1):
        super().__init__()
        self.beta = beta
        self.eps = _c.EPS

    def forward(self, logits, labels, type=0):
        return _avu(logits, labels, None, self.beta, True, type)


def entropy(prob):
    return _c.np_entropy(prob)


def predictive_entropy(mc_preds):
    """entropy of the MC-mean predictive distribution; mc_preds [S, batch, classes] probabilities"""
    return entropy(np.mean(mc_preds, axis=0))


def mutual_information(mc_preds):
    """H[mean_s p_s] - mean_s H[p_s]"""
    return entropy(np.mean(mc_preds, axis=0)) - np.mean(entropy(mc_preds), axis=0)


def eval_avu(pred_label, true_label, uncertainty):
    """(AvU [21], thresholds [21]): hard-count AvU at umin + t (umax - umin), t in np.linspace(0, 1, 21)"""
    t_list = np.linspace(0, 1, 21)
    umin = np.amin(uncertainty, axis=0)
    umax = np.amax(uncertainty, axis=0)
    u_th = umin + (t_list * (umax - umin))
    n_ac, n_au, n_ic, n_iu = _c.np_quadrant_counts(pred_label, true_label, uncertainty, u_th)
    return (n_ac + n_iu) / (n_ac + n_au + n_ic + n_iu + 1e-15), np.asarray(u_th)


def accuracy_vs_uncertainty(pred_label, true_label, uncertainty, optimal_threshold):
    """hard-count AvU at one threshold"""
    n_ac, n_au, n_ic, n_iu = _c.np_quadrant_counts(pred_label, true_label, uncertainty, optimal_threshold)
    return (n_ac + n_iu) / (n_ac + n_au + n_ic + n_iu)

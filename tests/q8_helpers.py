"""Shared by tests/test_q8_cpu.py and tests/test_gpu_q8.py: the INT8 fixtures (tests/golden/q8_*.npz, written by
tools/make_golden_q8.py from the reference) and builders of float layers / their quantized twins from them."""
import os

import numpy as np
import torch
import torch.nn as nn

import q8_model as Q

HERE = os.path.dirname(os.path.abspath(__file__))
SINGLE = ("q8_linear_default", "q8_conv_default", "q8_conv_stem_default", "q8_conv_fused_bn")
MAX_LSB, MAX_FRAC = 1, 0.005   # the issue's cap on |model - reference|: a condition of the fixtures, not a tolerance to tune

_CACHE = {}


def fixture(name):
    if name not in _CACHE:
        z = np.load(os.path.join(HERE, "golden", name + ".npz"))
        _CACHE[name] = {k: z[k] for k in z.files}
    return _CACHE[name]


def sub(d, prefix):
    return {k[len(prefix):]: v for k, v in d.items() if k.startswith(prefix)}


def geom(d):
    return {k: int(d[k]) for k in ("stride", "padding", "dilation") if k in d}


def model_record(d):
    """q8_model on one fixture record -> dict(W, S, b_i, acc, out)"""
    return Q.layer_forward(d["x_i"], int(d["z_x"]), float(d["s_x"]), d["mu_i"].astype(np.int32), float(d["s_mu"]),
                           d["sigma_i"].astype(np.int32), float(d["s_sigma"]), d["eps"], d.get("mu_b_q"), d.get("sigma_b_q"),
                           d.get("eps_b"), float(d["s_eps"]), float(d["s_d"]), float(d["s_w"]), float(d["s_o"]), int(d["z_o"]), **geom(d))


def assert_close_to_reference(out_i, d, what):
    diff = np.abs(np.asarray(out_i).astype(np.int32) - d["ref_out_i"].astype(np.int32))
    frac = float((diff != 0).mean())
    print("%s: max |diff| %d LSB, %d of %d elements differ (%.3f%%)" % (what, diff.max(), int((diff != 0).sum()), diff.size, 100 * frac))
    assert diff.max() <= MAX_LSB and frac <= MAX_FRAC, (what, int(diff.max()), frac)


def float_layer(d, conv, device="cpu"):
    """the float Reparameterization layer holding a record's parameters"""
    from bayesian_torch_amd import layers as L
    mu = torch.from_numpy(d["f_mu"])
    if conv:
        layer = L.Conv2dReparameterization(mu.shape[1], mu.shape[0], mu.shape[2], bias="f_mu_b" in d, **geom(d))
        wn = "kernel"
    else:
        layer = L.LinearReparameterization(mu.shape[1], mu.shape[0], bias="f_mu_b" in d)
        wn = "weight"
    with torch.no_grad():
        getattr(layer, "mu_" + wn).copy_(mu)
        getattr(layer, "rho_" + wn).copy_(torch.from_numpy(d["f_rho"]))
        if "f_mu_b" in d:
            layer.mu_bias.copy_(torch.from_numpy(d["f_mu_b"]))
            layer.rho_bias.copy_(torch.from_numpy(d["f_rho_b"]))
    return layer.to(device)


class Block(nn.Module):
    """conv1 (+ bn1): what bnn_to_qbnn(fuse_conv_bn=True) folds"""

    def __init__(self, conv, bn=None):
        super().__init__()
        self.conv1 = conv
        if bn is not None:
            self.bn1 = bn


def bn_of(d):
    bn = nn.BatchNorm2d(d["bn_weight"].shape[0], eps=float(d["bn_eps"]))
    with torch.no_grad():
        bn.weight.copy_(torch.from_numpy(d["bn_weight"]))
        bn.bias.copy_(torch.from_numpy(d["bn_bias"]))
        bn.running_mean.copy_(torch.from_numpy(d["bn_mean"]))
        bn.running_var.copy_(torch.from_numpy(d["bn_var"]))
    return bn.eval()


def quantized_layer(d, device="cpu"):
    """the twin models.bnn_to_qbnn builds from a single-layer fixture record (with its quant_dict when it was calibrated)"""
    from bayesian_torch_amd.models import bnn_to_qbnn
    conv = int(d["kind"]) == 1
    m = Block(float_layer(d, conv), bn_of(d) if "bn_weight" in d else None).to(device)
    bnn_to_qbnn(m, fuse_conv_bn="bn_weight" in d)
    return m.conv1


def quant_dict_of(d):
    return [(float(d["s_eps"]), 0), (float(d["s_d"]), 0), (float(d["s_w"]), 0), (float(d["s_x"]), int(d["z_x"])),
            (float(d["s_o"]), int(d["z_o"]))]

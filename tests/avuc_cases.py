"""tests/golden/avuc.npz (tools/make_golden_avuc.py: inputs and the reference's own outputs) and the float64 truth shared by
test_avuc_cpu.py and test_gpu_avuc.py."""
import functools
import os

import numpy as np
import torch

from bayesian_torch_amd.utils import _calibration as C

HERE = os.path.dirname(os.path.abspath(__file__))


@functools.lru_cache(maxsize=None)
def load():
    z = np.load(os.path.join(HERE, "golden", "avuc.npz"))
    out = {"avu": {}, "eau": {}, "np": {}}
    for key in z.files:
        parts = key.split("/")
        if parts[0] == "np":
            out["np"][parts[1]] = z[key]
        else:
            out[parts[0]].setdefault(parts[1], {})[parts[2]] = z[key]
    return out


AVU_NAMES = ("b7_c10", "b37_c257", "b64_c1000", "b1500_c10", "b5_c4100", "b1_c10", "bf16_b7_c10", "bf16_b37_c257")
AREA_NAMES = tuple(n for n in AVU_NAMES if n != "b1_c10")
F32_AREA_NAMES = tuple(n for n in AREA_NAMES if not n.startswith("bf16_"))
EAU_NAMES = ("e7", "e37", "e1500")


def _f(v):
    return float(v.detach()) if torch.is_tensor(v) else float(v)


def rel(a, b):
    return abs(_f(a) - _f(b)) / max(abs(_f(b)), 1e-30)


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def max_over_max(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def avu_run(logits, labels, th, beta, area, dtype):
    """the ATen chain on the CPU in `dtype`: (loss, r, dlogits of loss) as numpy"""
    lg = torch.as_tensor(logits).to(dtype).clone().requires_grad_(True)
    loss, r = C.avu_chain(lg, torch.as_tensor(labels), float(th), float(beta), area)
    loss.backward()
    return loss.detach().numpy().reshape(-1)[0], r.detach().numpy().reshape(-1)[0], lg.grad.numpy()


def eau_run(error, other, e_th, o_th, beta, conf_form, dtype):
    e = torch.as_tensor(error).to(dtype).clone().requires_grad_(True)
    o = torch.as_tensor(other).to(dtype).clone().requires_grad_(True)
    loss = C.eau_chain(e, o, float(e_th), float(o_th), float(beta), conf_form)
    loss.backward()
    return loss.detach().numpy().reshape(-1)[0], e.grad.numpy(), o.grad.numpy()


@functools.lru_cache(maxsize=None)
def avu_truth(name, area):
    """float64 chain and the error of the float32 chain against it: dict(loss, r, grad, e32_loss, e32_l2, e32_max)"""
    c = load()["avu"][name]
    l64, r64, g64 = avu_run(c["logits"], c["labels"], c["th"], c["beta"], area, torch.float64)
    l32, r32, g32 = avu_run(c["logits"], c["labels"], c["th"], c["beta"], area, torch.float32)
    return dict(loss=l64, r=r64, grad=g64, e32_loss=rel(l32, l64), e32_l2=rel_l2(g32, g64), e32_max=max_over_max(g32, g64))


@functools.lru_cache(maxsize=None)
def eau_truth(name, conf_form):
    c = load()["eau"][name]
    other, o_th = (c["conf"], c["conf_th"]) if conf_form else (c["unc"], c["unc_th"])
    l64, de64, do64 = eau_run(c["error"], other, c["error_th"], o_th, c["beta"], conf_form, torch.float64)
    l32, de32, do32 = eau_run(c["error"], other, c["error_th"], o_th, c["beta"], conf_form, torch.float32)
    g64, g32 = np.concatenate([de64, do64]), np.concatenate([de32, do32])
    return dict(loss=l64, derror=de64, dother=do64, e32_loss=rel(l32, l64), e32_l2=rel_l2(g32, g64),
                e32_max=max_over_max(g32, g64))


def assert_avu_margin(name, area):
    """the fixture's margins, re-derived from the float64 chain: a missing margin is a failure"""
    c = load()["avu"][name]
    lg = torch.as_tensor(c["logits"]).double()
    conf, pred, ent = C.row_stats(lg)
    top2 = torch.topk(torch.softmax(lg, 1), 2, dim=1).values
    assert float((top2[:, 0] - top2[:, 1]).min()) > 1e-3, name
    m = float(c["margin"])
    if area:
        d = (ent.unsqueeze(0) - C.area_thresholds(ent).unsqueeze(1)).abs()
        d[0, ent.argmin()] = float("inf")
        d[C.N_THRESHOLDS - 1, ent.argmax()] = float("inf")
        assert float(d.min()) > m, name
    else:
        assert float((ent - float(c["th"])).abs().min()) > m, name


def assert_eau_margin(name):
    c = load()["eau"][name]
    for v, t in (("error", "error_th"), ("unc", "unc_th"), ("conf", "conf_th")):
        assert float(np.abs(c[v].astype(np.float64) - float(c[t])).min()) > 1e-3, (name, v)

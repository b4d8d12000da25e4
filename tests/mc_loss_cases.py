"""Cases and float64 truth shared by test_mc_loss_cpu.py and test_gpu_mc_loss.py: Monte-Carlo stacked logits [S, B, C] from a seeded
numpy generator (no golden file), the float64 ATen chains of utils/mc_loss.py and utils/_calibration.py as the oracle, and the error
of the float32 CPU chain against it (the yardstick of tests/test_gpu_avuc.py's tolerance rule).

Logits: a base row per example times `scale`, plus per-sample offsets of half that scale, so the samples disagree and the mutual
information is not vanishing; values are rounded to bf16 for the bf16 cases (exact in the fixture).  The `wide` cases slice C = 1001
columns out of a wider buffer on the device: rows off the 16-byte grid.  Half of the labels are the prediction of the mean
distribution, so good and bad quadrants are both populated.

AvUC cases re-assert their margins from the float64 chain before anything is compared (as tests/avuc_cases.py does): no example's
mutual information within 1e-3 of a threshold it is compared with, top-2 gap of pbar above 1e-3.  The seeds below were picked so
that this holds; test_mc_loss_cpu.py checks every one of them."""
import functools

import numpy as np
import torch

from bayesian_torch_amd.utils import _calibration as C
from bayesian_torch_amd.utils import mc_loss as M

MARGIN = 1e-3

# name: (S, B, C, scale, dtype, seed)
CE_CASES = {
    "s1_b3_c10_x1": (1, 3, 10, 1, "f32", 101),
    "s2_b1_c2_x8": (2, 1, 2, 8, "f32", 102),
    "s2_b37_c10_x1": (2, 37, 10, 1, "f32", 103),
    "s2_b65_c2_x1": (2, 65, 2, 1, "f32", 104),
    "s5_b65_c257_x8": (5, 65, 257, 8, "f32", 105),
    "s5_b3_c1000_x1": (5, 3, 1000, 1, "f32", 106),
    "s32_b37_c10_x8": (32, 37, 10, 8, "f32", 107),
    "s32_b1_c1000_x1": (32, 1, 1000, 1, "f32", 108),
    "s1_b65_c1000_x8": (1, 65, 1000, 8, "f32", 109),
    "s5_b3_c1001_x8_wide": (5, 3, 1001, 8, "f32", 110),
    "bf16_s5_b37_c1000_x8": (5, 37, 1000, 8, "bf16", 111),
    "bf16_s2_b3_c257_x1": (2, 3, 257, 1, "bf16", 112),
    "bf16_s5_b3_c1001_x8_wide": (5, 3, 1001, 8, "bf16", 113),
}
# AvUC: scale 8 so the mutual information spreads.  Two classes (the uncertainties of agreeing samples pile up at 0) and scale 1 (all
# uncertainties within a few 1e-2) cannot keep 1e-3 from 21 thresholds: those two cases take the single threshold only, at B = 3.
AVU_CASES = {
    "s2_b3_c10_x8": (2, 3, 10, 8, "f32", 301),
    "s5_b37_c257_x8": (5, 37, 257, 8, "f32", 202),
    "s32_b65_c10_x8": (32, 65, 10, 8, "f32", 603),
    "s5_b65_c1000_x8": (5, 65, 1000, 8, "f32", 604),
    "s2_b3_c2_x8": (2, 3, 2, 8, "f32", 205),
    "s5_b1_c10_x8": (5, 1, 10, 8, "f32", 206),
    "s2_b3_c10_x1": (2, 3, 10, 1, "f32", 207),
    "s5_b3_c1001_x8_wide": (5, 3, 1001, 8, "f32", 208),
    "s2_b3_c16128_x8": (2, 3, 16128, 8, "f32", 211),  # the widest row the type=1 kernels take (_calibration.AVU_MC_MAX_CLASSES)
    "bf16_s5_b37_c1000_x8": (5, 37, 1000, 8, "bf16", 409),
    "bf16_s5_b3_c1001_x8_wide": (5, 3, 1001, 8, "bf16", 210),
}
AVU_AREA_CASES = tuple(n for n, c in AVU_CASES.items() if c[1] > 1 and c[2] > 2 and c[3] == 8)
S1_CASE = (1, 37, 10, 8, "f32", 301)
BETA = 3.0
KL = 1234.5
SMOOTHING = (0.0, 0.1)
REDUCES = ("logits", "loss")


def make(spec):
    """dict(stack f32 numpy [S, B, C], labels int64 [B], th) of one case; bf16 cases hold values exact in bf16"""
    S, B, Cn, scale, dtype, seed = spec
    rng = np.random.default_rng(seed)
    base = rng.standard_normal((B, Cn)) * scale
    stack = (base[None] + 0.5 * scale * rng.standard_normal((S, B, Cn))).astype(np.float32)
    if dtype == "bf16":
        stack = torch.from_numpy(stack).to(torch.bfloat16).float().numpy()
    conf, pred, unc = C.mc_row_stats(torch.from_numpy(stack).double())
    labels = rng.integers(0, Cn, B).astype(np.int64)
    hit = rng.random(B) < 0.5
    labels[hit] = pred.numpy()[hit]
    u = np.sort(unc.numpy())
    if B == 1:
        th = float(u[0] + 0.1)
    else:  # the middle of the widest gap of the sorted uncertainties: examples on both sides
        i = int(np.argmax(np.diff(u)))
        th = float(0.5 * (u[i] + u[i + 1]))
    th = float(np.float32(th))  # exact in f32: a Python-number and a tensor threshold are then the same number on the device
    return dict(stack=stack, labels=labels, th=th, wide=is_wide(spec))


def is_wide(spec):
    return spec[2] == 1001  # the C = 1001 cases live in a wider buffer on the device (to_device)


@functools.lru_cache(maxsize=None)
def ce_case(name):
    return make(CE_CASES[name])


@functools.lru_cache(maxsize=None)
def avu_case(name):
    return make(AVU_CASES[name])


@functools.lru_cache(maxsize=None)
def s1_case():
    return make(S1_CASE)


def torch_dtype(name):
    return torch.bfloat16 if name.startswith("bf16_") else torch.float32


def to_device(c, dev, dtype):
    """(stack, labels) on `dev`; a `wide` case is a slice of a buffer with 7 more columns, starting at column 3: no row on the
    16-byte grid"""
    st = torch.from_numpy(c["stack"]).to(dev).to(dtype)
    if c["wide"]:
        S, B, Cn = st.shape
        buf = torch.zeros(S, B, Cn + 7, dtype=dtype, device=dev)
        buf[:, :, 3:3 + Cn] = st
        st = buf[:, :, 3:3 + Cn]
    return st, torch.from_numpy(c["labels"]).to(dev)


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


def ce_run(c, reduce, ls, dtype, kl=KL):
    """the ATen chain on the CPU in `dtype`: (loss, dstack, dkl) as numpy"""
    st = torch.from_numpy(c["stack"]).to(dtype).clone().requires_grad_(True)
    k = torch.tensor(kl, dtype=dtype, requires_grad=True)
    loss = M._mc_ce_chain(st, torch.from_numpy(c["labels"]), k, reduce, ls)
    loss.backward()
    return float(loss.detach()), st.grad.numpy(), float(k.grad)


def avu_run(c, th, area, dtype):
    st = torch.from_numpy(c["stack"]).to(dtype).clone().requires_grad_(True)
    loss, r = C.avu_mc_chain(st, torch.from_numpy(c["labels"]), float(th), BETA, area)
    loss.backward()
    return float(loss.detach()), float(r.detach()), st.grad.numpy()


def _truth(run):
    l64, g64 = run(torch.float64)
    l32, g32 = run(torch.float32)
    return dict(loss=l64, grad=g64, e32_loss=rel(l32, l64), e32_l2=rel_l2(g32, g64), e32_max=max_over_max(g32, g64))


@functools.lru_cache(maxsize=None)
def ce_truth(name, reduce, ls):
    """float64 chain and the error of the float32 CPU chain against it"""
    c = ce_case(name)
    return _truth(lambda dt: ce_run(c, reduce, ls, dt)[:2])


@functools.lru_cache(maxsize=None)
def avu_truth(name, area):
    c = avu_case(name)

    def run(dt):
        loss, _, g = avu_run(c, c["th"], area, dt)
        return loss, g
    t = _truth(run)
    t["r"] = avu_run(c, c["th"], area, torch.float64)[1]
    return t


def assert_avu_margin(name, area):
    """the case's margins, re-derived from the float64 chain: a missing margin is a failure"""
    c = avu_case(name)
    st = torch.from_numpy(c["stack"]).double()
    conf, pred, unc = C.mc_row_stats(st)
    if st.shape[2] > 1:
        top2 = torch.topk(torch.softmax(st, 2).mean(0), 2, dim=1).values
        assert float((top2[:, 0] - top2[:, 1]).min()) > MARGIN, name
    if area:
        d = (unc.unsqueeze(0) - C.area_thresholds(unc).unsqueeze(1)).abs()
        d[0, unc.argmin()] = float("inf")
        d[C.N_THRESHOLDS - 1, unc.argmax()] = float("inf")
        assert float(d.min()) > MARGIN, (name, float(d.min()))
    else:
        assert float((unc - c["th"]).abs().min()) > MARGIN, (name, float((unc - c["th"]).abs().min()))

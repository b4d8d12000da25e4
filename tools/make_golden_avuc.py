#!/usr/bin/env python3
"""Generate tests/golden/avuc.npz by running the REFERENCE calibration losses (IntelLabs/bayesian-torch,
bayesian_torch/utils/avuc_loss.py and uncertainty_calibration_loss.py) on the CPU and freezing inputs and outputs.

usage: python tools/make_golden_avuc.py --reference /path/to/bayesian-torch     (needs scikit-learn, as the reference does)

The losses are discontinuous where an example crosses a threshold, so a fixture is only worth anything when no example is
near one.  For every case the generator searches seeds and ASSERTS, before it stores anything:
  * every |H_i - th| > margin for the single threshold and for the 21 thresholds of the area form (margin 1e-3; 1e-4 for
    B = 1500), the umin / umax examples at k = 0 / k = 20 excepted;
  * the gap between the two largest probabilities of every row > 1e-3 (the prediction does not depend on rounding);
  * for EaU / EaC every input at least 1e-3 away from its threshold;
  * for the area form, the reference's own top threshold (umin + 1 * (umax - umin), umax - umin rounded in f32) >= umax, so
    that its auc_avu() equals the intended value (the most uncertain example is certain at t = 1).
Stored thresholds are exact in float32.  Cases named bf16_* have logits that are exact in bfloat16.
"""
import argparse
import os
import sys
import warnings

import numpy as np
import torch

warnings.filterwarnings("ignore")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name, B, C, scale of randn, beta, margin, bf16-exact logits
AVU_CASES = [
    ("b7_c10", 7, 10, 2.0, 1.0, 1e-3, False),
    ("b37_c257", 37, 257, 3.0, 3.0, 1e-3, False),
    ("b64_c1000", 64, 1000, 3.0, 1.0, 1e-3, False),
    ("b1500_c10", 1500, 10, 2.0, 0.5, 1e-4, False),
    ("b5_c4100", 5, 4100, 4.0, 1.0, 1e-3, False),
    ("b1_c10", 1, 10, 2.0, 1.0, 1e-3, False),          # avuc_loss.AvULoss only: B == 1 is degenerate in the other forms
    ("bf16_b7_c10", 7, 10, 2.0, 1.0, 1e-3, True),
    ("bf16_b37_c257", 37, 257, 3.0, 3.0, 1e-3, True),
]
# name, B, beta
EAU_CASES = [("e7", 7, 1.0), ("e37", 37, 3.0), ("e1500", 1500, 0.5)]
MAX_TRIES = 400


def entropy64(logits):
    p = torch.softmax(logits.double(), dim=1)
    return -(p * torch.log(p + 1e-10)).sum(-1), p


def pick_threshold(values, margin):
    """midpoint (rounded to f32) of the widest gap between neighbours in the central half of `values`, or None"""
    v = np.sort(np.asarray(values, dtype=np.float64))
    if v.size == 1:
        th = float(np.float32(v[0] + 0.25))
        return th if abs(th - v[0]) > margin else None
    lo, hi = v.size // 4, max(v.size // 4 + 1, (3 * v.size) // 4)
    gaps = v[lo + 1:hi + 1] - v[lo:hi]
    j = int(np.argmax(gaps)) + lo
    th = float(np.float32(0.5 * (v[j] + v[j + 1])))
    return th if np.min(np.abs(v - th)) > margin else None


def area_margin(H, margin):
    """min |H_i - th_k| over the 21 exact thresholds, the umin / umax examples at k = 0 / k = 20 excepted"""
    h = H.numpy()
    umin, umax = h.min(), h.max()
    th = umin + np.arange(21) * 0.05 * (umax - umin)
    th[20] = umax
    d = np.abs(h[None, :] - th[:, None])
    d[0, np.argmin(h)] = np.inf
    d[20, np.argmax(h)] = np.inf
    return d.min()


def ref_top_threshold_reaches_umax(logits):
    """the reference's arithmetic at t = 1 (avuc_loss.py:235: a float64 0-d tensor times the f32-rounded umax - umin)"""
    p = torch.softmax(logits, dim=1)
    unc = -1 * torch.sum(p * torch.log(p + 1e-10), dim=-1)
    umin, umax = torch.min(unc), torch.max(unc)
    return (umin + (torch.tensor(np.float64(1.0)) * (umax - umin))).item() >= umax.item()


def make_avu_case(name, B, C, scale, beta, margin, bf16, ref_avuc, ref_ucl):
    for seed in range(MAX_TRIES):
        g = torch.Generator().manual_seed(seed)
        logits = torch.randn(B, C, generator=g) * scale
        if bf16:
            logits = logits.bfloat16().float()
        labels = torch.randint(0, C, (B,), generator=g)
        labels[::2] = logits.argmax(1)[::2]  # half the examples accurate
        H, p = entropy64(logits)
        top2 = torch.topk(p, 2, dim=1).values
        if float((top2[:, 0] - top2[:, 1]).min()) <= 1e-3:
            continue
        th = pick_threshold(H.numpy(), margin)
        if th is None:
            continue
        if B > 1:
            if area_margin(H, margin) <= margin:
                continue
            if not ref_top_threshold_reaches_umax(logits):
                continue
        break
    else:
        raise SystemExit("%s: no seed with the margins in %d tries" % (name, MAX_TRIES))
    # the margins, asserted on what is stored
    assert float((top2[:, 0] - top2[:, 1]).min()) > 1e-3
    assert float((H - th).abs().min()) > margin
    out = {"logits": logits.numpy(), "labels": labels.numpy(), "th": np.float32(th), "beta": np.float32(beta),
           "margin": np.float32(margin), "seed": np.int64(seed)}
    lg = logits.clone().requires_grad_(True)
    loss = ref_avuc.AvULoss(beta=beta)(lg, labels, th)
    loss.backward()
    out["ref1_loss"] = loss.detach().numpy().reshape(1)
    out["ref1_dlogits"] = lg.grad.numpy().copy()
    if B > 1:
        assert area_margin(H, margin) > margin
        lg = logits.clone().requires_grad_(True)
        loss = ref_ucl.AvULoss(beta=beta)(lg, labels, th)
        loss.backward()
        out["ref2_loss"] = loss.detach().numpy().reshape(1)
        # stored as the difference from ref1 (exact to undo in f32: the two agree to a few ulps), which compresses to nothing
        d2 = lg.grad.numpy()
        diff = d2 - out["ref1_dlogits"]
        assert np.array_equal(out["ref1_dlogits"] + diff, d2)
        out["ref2_dlogits_minus_ref1"] = diff
        area = ref_avuc.AUAvULoss(beta=beta)
        with torch.no_grad():
            unc = area.entropy(torch.softmax(logits, dim=1))
            assert ref_top_threshold_reaches_umax(logits)
            out["ref_auc"] = np.float64(np.asarray(area.auc_avu(logits, labels, unc)).reshape(-1)[0])
    print("%-14s seed %3d  th %.6f  ref loss %.7f%s" % (name, seed, th, float(out["ref1_loss"][0]),
                                                        "  auc %.7f" % out["ref_auc"] if B > 1 else ""))
    return out


def make_eau_case(name, B, beta, ref_ucl):
    for seed in range(MAX_TRIES):
        g = torch.Generator().manual_seed(1000 + seed)
        error = torch.randn(B, generator=g).abs()
        unc = torch.randn(B, generator=g).abs() * 0.7
        conf = torch.rand(B, generator=g)
        ths = [pick_threshold(v.numpy(), 1e-3) for v in (error, unc, conf)]
        if all(t is not None for t in ths):
            break
    else:
        raise SystemExit("%s: no seed with the margins in %d tries" % (name, MAX_TRIES))
    e_th, u_th, c_th = ths
    for v, t in ((error, e_th), (unc, u_th), (conf, c_th)):
        assert float((v.double() - t).abs().min()) > 1e-3
    out = {"error": error.numpy(), "unc": unc.numpy(), "conf": conf.numpy(), "error_th": np.float32(e_th),
           "unc_th": np.float32(u_th), "conf_th": np.float32(c_th), "beta": np.float32(beta)}
    for key, cls, other, o_th in (("eau", ref_ucl.EaULoss, unc, u_th), ("eac", ref_ucl.EaCLoss, conf, c_th)):
        e = error.clone().requires_grad_(True)
        o = other.clone().requires_grad_(True)
        loss = cls(beta=beta)(e, o, e_th, o_th)
        loss.backward()
        out[key + "_loss"] = loss.detach().numpy().reshape(1)
        out[key + "_derror"] = e.grad.numpy().copy()
        out[key + "_dother"] = o.grad.numpy().copy()
    print("%-14s seed %3d  eau %.7f  eac %.7f" % (name, seed, float(out["eau_loss"][0]), float(out["eac_loss"][0])))
    return out


def make_numpy_case(ref_avuc):
    for seed in range(MAX_TRIES):
        rs = np.random.RandomState(seed)
        z = rs.randn(4, 9, 6) * 2
        mc = np.exp(z) / np.exp(z).sum(-1, keepdims=True)
        unc = ref_avuc.predictive_entropy(mc)
        pred = mc.mean(0).argmax(-1)
        true = pred.copy()
        true[1::2] = (true[1::2] + 1) % 6
        umin, umax = unc.min(), unc.max()
        th = umin + np.linspace(0, 1, 21) * (umax - umin)
        d = np.abs(unc[None] - th[:, None])
        d[0, unc.argmin()] = np.inf
        d[20, unc.argmax()] = np.inf
        if d.min() > 1e-3 and th[20] >= umax:
            break
    else:
        raise SystemExit("numpy helpers: no seed")
    avu, ths = ref_avuc.eval_avu(pred, true, unc)
    th1 = float(0.5 * (np.sort(unc)[4] + np.sort(unc)[5]))
    return {"mc_preds": mc, "pred": pred, "true": true, "entropy": ref_avuc.entropy(mc),
            "predictive_entropy": unc, "mutual_information": ref_avuc.mutual_information(mc), "eval_avu": avu,
            "eval_avu_th": ths, "th": np.float64(th1),
            "accuracy_vs_uncertainty": np.float64(ref_avuc.accuracy_vs_uncertainty(pred, true, unc, th1))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of IntelLabs/bayesian-torch")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "avuc.npz"))
    a = ap.parse_args()
    sys.path.insert(0, a.reference)
    import bayesian_torch.utils.avuc_loss as ref_avuc
    import bayesian_torch.utils.uncertainty_calibration_loss as ref_ucl
    torch.set_num_threads(1)
    store = {}
    for case in AVU_CASES:
        for k, v in make_avu_case(*case, ref_avuc, ref_ucl).items():
            store["avu/%s/%s" % (case[0], k)] = v
    for case in EAU_CASES:
        for k, v in make_eau_case(*case, ref_ucl).items():
            store["eau/%s/%s" % (case[0], k)] = v
    for k, v in make_numpy_case(ref_avuc).items():
        store["np/%s" % k] = v
    np.savez_compressed(a.out, **store)
    print("wrote %s: %d bytes" % (a.out, os.path.getsize(a.out)))
    assert os.path.getsize(a.out) < 1000000


if __name__ == "__main__":
    main()

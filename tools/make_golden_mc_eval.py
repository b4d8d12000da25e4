#!/usr/bin/env python3
"""Generate tests/golden/mc_eval.npz: MC logits, labels and what the REFERENCE's evaluation code (IntelLabs/bayesian-torch:
examples/main_bayesian_imagenet.py evaluate(), bayesian_torch/utils/util.py, bayesian_torch/utils/avuc_loss.py) makes of them.

usage: python tools/make_golden_mc_eval.py --reference /path/to/bayesian-torch

Four cases (S, B, C).  Logits: a base randn * scale shared by the samples plus 0.7 * randn per sample, rounded to values exact
in float16 (stored as float16: the largest case would not fit the size limit of a committed file in float32; the tests widen
them back, so they ARE the f32 logits).  Labels: random, every second row the argmax of the mean logits.

Every integer decision a test compares exactly must not hang on a rounding, so before anything is written the generator ASSERTS:
  * relative gap of the two largest mean probabilities of every row >= 1e-4;
  * relative gap between p_y and every other p_c >= 1e-4;
  * |conf * 15 - round(conf * 15)| >= 1e-4;
  * every entropy at least 1e-4 away from the three stored interior thresholds and from eval_avu's interior thresholds.
If a seed fails an assertion, change the seed, not the margin.
"""
import argparse
import os
import sys
import warnings

import numpy as np
import torch

warnings.filterwarnings("ignore")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name, S, B, C, scale of the shared base, numpy default_rng seed
CASES = [("s8_b48_c10", 8, 48, 10, 2.0, 1), ("s4_b7_c1000", 4, 7, 1000, 3.0, 2), ("s20_b64_c257", 20, 64, 257, 3.0, 3),
         ("s5_b33_c2", 5, 33, 2, 1.5, 4)]
MARGIN = 1e-4
NBINS = 15


def interior_thresholds(H):
    """three thresholds (exact in f32) in the widest gaps around the quartiles of H"""
    v = np.sort(H)
    out = []
    for q in (0.25, 0.5, 0.75):
        j0 = int(q * (v.size - 1))
        lo, hi = max(j0 - 2, 0), min(j0 + 2, v.size - 2)
        j = lo + int(np.argmax(v[lo + 1:hi + 2] - v[lo:hi + 1]))
        out.append(np.float32(0.5 * (v[j] + v[j + 1])))
    return np.asarray(out, np.float32)


def make_case(name, S, B, C, scale, seed, util, avuc):
    r = np.random.default_rng(seed)
    base = r.standard_normal((B, C)) * scale
    logits = (base[None] + 0.7 * r.standard_normal((S, B, C))).astype(np.float16)
    lg = torch.from_numpy(logits.astype(np.float32))
    labels = r.integers(0, C, B)
    labels[::2] = lg.mean(0).argmax(1).numpy()[::2]
    # the reference's evaluate(): softmax per sample, np.mean over the samples, argmax, accuracy
    probs = torch.softmax(lg, dim=-1).numpy()
    mean = np.mean(probs, axis=0)
    pred = np.argmax(mean, axis=-1)
    acc = np.mean(pred == labels)
    p64 = probs.astype(np.float64)
    H = util.predictive_entropy(p64)
    MI = util.mutual_information(p64)
    avu, avu_th = avuc.eval_avu(pred, labels, H)
    k = min(5, C)
    top5 = (torch.topk(torch.from_numpy(mean), k, dim=1).indices.numpy() == labels[:, None]).any(1)
    th3 = interior_thresholds(H)
    # margins
    m64 = p64.mean(0)
    srt = np.sort(m64, axis=1)
    if C > 1:
        assert ((srt[:, -1] - srt[:, -2]) / srt[:, -1]).min() >= MARGIN, name
        py = m64[np.arange(B), labels]
        gap = np.abs(m64 - py[:, None]) / np.maximum(m64, py[:, None])
        gap[np.arange(B), labels] = np.inf
        assert gap.min() >= MARGIN, name
    conf = m64.max(1)
    assert np.abs(conf * NBINS - np.round(conf * NBINS)).min() >= MARGIN, name
    assert np.abs(H[None, :] - th3[:, None].astype(np.float64)).min() >= MARGIN, name
    assert np.abs(H[None, :] - avu_th[1:-1, None]).min() >= MARGIN, name
    hit = pred == labels
    cert = H[None, :] <= th3[:, None].astype(np.float64)
    quad = np.stack([(hit & cert).sum(1), (hit & ~cert).sum(1), (~hit & cert).sum(1), (~hit & ~cert).sum(1)], 1)
    b = np.clip(np.ceil(conf * NBINS).astype(np.int64) - 1, 0, NBINS - 1)
    bins = np.stack([np.bincount(b, minlength=NBINS), np.bincount(b[hit], minlength=NBINS)], 1)
    print("%-14s acc %.4f  top5 %.4f  mean H %.4f  mean MI %.4f" % (name, acc, top5.mean(), H.mean(), MI.mean()))
    return {"logits": logits, "labels": labels.astype(np.int64), "pred": pred.astype(np.int64), "accuracy": np.float64(acc),
            "top5": top5, "H": H, "MI": MI, "eval_avu": avu, "eval_avu_th": avu_th, "th3": th3, "quad3": quad.astype(np.int64),
            "bin_count_hits": bins.astype(np.int64)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of IntelLabs/bayesian-torch")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "mc_eval.npz"))
    a = ap.parse_args()
    sys.path.insert(0, a.reference)
    import bayesian_torch.utils.util as util
    import bayesian_torch.utils.avuc_loss as avuc
    torch.set_num_threads(1)
    store = {}
    for case in CASES:
        for k, v in make_case(*case, util, avuc).items():
            store["%s/%s" % (case[0], k)] = v
    np.savez_compressed(a.out, **store)
    print("wrote %s: %d bytes" % (a.out, os.path.getsize(a.out)))
    assert os.path.getsize(a.out) < 1000000


if __name__ == "__main__":
    main()

"""Measures the error of the device's f32 exp and log, in ulps of the result, over the ranges the regression heads use
(tests/reg_model.py: C_EXP_ULP / C_LOG_ULP are 2 x these maxima):

    torch.exp on [-8, 8]           s ~ U[-3, 3] in the tests, with room for log-variances a model actually predicts
    torch.log on [2^-12, 2^12]     sums of such variances and 2 pi var

f32, 4 M points each (uniform in x for exp, uniform in log2 x for log), against float64 on the same device.

    python tools/reg_envelope.py [--out profiles/reg_envelope.txt] [--points 4194304]
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def ulp32(v):
    """spacing of f32 at |v| (float64 tensor)"""
    a = v.abs().clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(a)) - 23)


def worst(fn, x):
    got = fn(x).double()
    ref = fn(x.double())
    err = (got - ref).abs() / ulp32(ref)
    i = int(err.argmax())
    return float(err[i]), float(x[i])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reg_envelope.txt"))
    ap.add_argument("--points", type=int, default=1 << 22)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "reg_envelope.py measures on the GPU only"
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    xe = (torch.rand(a.points, generator=g, device=dev, dtype=torch.float64) * 16 - 8).float()
    xl = torch.exp2(torch.rand(a.points, generator=g, device=dev, dtype=torch.float64) * 24 - 12).float()
    e, ex = worst(torch.exp, xe)
    l, lx = worst(torch.log, xl)
    lines = ["python tools/reg_envelope.py " + " ".join(sys.argv[1:]),
             "device: %s, torch %s; %d points each, f32 against float64 on the device, error in ulps of the float64 result" % (
                 torch.cuda.get_device_name(0), torch.__version__, a.points),
             "exp on [-8, 8]: max %.3f ulp at x = %.9g" % (e, ex),
             "log on [2^-12, 2^12]: max %.3f ulp at x = %.9g" % (l, lx),
             "tests/reg_model.py: C_EXP_ULP = %.2f, C_LOG_ULP = %.2f (2 x the maxima, rounded up)" % (
                 -(-2 * e * 100 // 1) / 100, -(-2 * l * 100 // 1) / 100)]
    print("\n".join(lines))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

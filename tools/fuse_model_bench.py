"""ms per MC sample of a VGG16-BN-shaped and a MobileNetV2-shaped model, converted by dnn_to_bnn, with and without
models.fuse.fuse_model, replayed by mc.GraphedMC with MC samples as lanes of one launch per layer.

    python tools/fuse_model_bench.py [--type Flipout] [--bs 64] [--lanes 8] [--replays 6] [--models vgg16_bn,mobilenet_v2]

bf16 activations at 224 x 224 (the BN layers in bf16 too, the variational parameters f32, as bench.py runs ResNet18).  Prints one
JSON line per (model, fused).  The models are defined here (the torchvision layer lists, no torchvision import)."""
import argparse
import json
import os
import sys
import time

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PRIOR = dict(prior_mu=0.0, prior_sigma=1.0, posterior_mu_init=0.0, posterior_rho_init=-3.0, moped_enable=False, moped_delta=0.5)


def vgg16_bn(classes=1000):
    """13 conv-BN-ReLU (64, 64, M, 128, 128, M, 256 x3, M, 512 x3, M, 512 x3, M), then Linear-BN1d-ReLU x2 and the classifier"""
    cfg = [64, 64, "M", 128, 128, "M", 256, 256, 256, "M", 512, 512, 512, "M", 512, 512, 512, "M"]
    layers, cin = [], 3
    for v in cfg:
        if v == "M":
            layers.append(nn.MaxPool2d(2, 2))
        else:
            layers += [nn.Conv2d(cin, v, 3, padding=1), nn.BatchNorm2d(v), nn.ReLU(inplace=True)]
            cin = v
    return nn.Sequential(nn.Sequential(*layers), nn.Flatten(),
                         nn.Linear(512 * 7 * 7, 4096), nn.BatchNorm1d(4096), nn.ReLU(inplace=True),
                         nn.Linear(4096, 4096), nn.BatchNorm1d(4096), nn.ReLU(inplace=True), nn.Linear(4096, classes))


class _InvRes(nn.Module):
    def __init__(self, cin, cout, stride, t):
        super().__init__()
        hid = cin * t
        self.skip = stride == 1 and cin == cout
        layers = []
        if t != 1:
            layers += [nn.Conv2d(cin, hid, 1, bias=False), nn.BatchNorm2d(hid), nn.ReLU6(inplace=True)]
        layers += [nn.Conv2d(hid, hid, 3, stride, 1, groups=hid, bias=False), nn.BatchNorm2d(hid), nn.ReLU6(inplace=True),
                   nn.Conv2d(hid, cout, 1, bias=False), nn.BatchNorm2d(cout)]
        self.conv = nn.Sequential(*layers)

    def forward(self, x):
        return x + self.conv(x) if self.skip else self.conv(x)


class MobileNetV2(nn.Module):
    """the MobileNetV2 layer list (width 1.0): stem ConvBNReLU6, 17 inverted residuals, 1x1 ConvBNReLU6 to 1280, classifier"""

    def __init__(self, classes=1000):
        super().__init__()
        setting = [(1, 16, 1, 1), (6, 24, 2, 2), (6, 32, 3, 2), (6, 64, 4, 2), (6, 96, 3, 1), (6, 160, 3, 2), (6, 320, 1, 1)]
        feats, cin = [nn.Sequential(nn.Conv2d(3, 32, 3, 2, 1, bias=False), nn.BatchNorm2d(32), nn.ReLU6(inplace=True))], 32
        for t, c, n, s in setting:
            for i in range(n):
                feats.append(_InvRes(cin, c, s if i == 0 else 1, t))
                cin = c
        feats.append(nn.Sequential(nn.Conv2d(cin, 1280, 1, bias=False), nn.BatchNorm2d(1280), nn.ReLU6(inplace=True)))
        self.features = nn.Sequential(*feats)
        self.classifier = nn.Linear(1280, classes)

    def forward(self, x):
        x = self.features(x)
        return self.classifier(torch.flatten(nn.functional.adaptive_avg_pool2d(x, 1), 1))


MODELS = {"vgg16_bn": vgg16_bn, "mobilenet_v2": MobileNetV2}


def build(name, typ, dev, fuse):
    import bayesian_torch_amd as bt
    from bayesian_torch_amd.models import dnn_to_bnn, fuse_model
    torch.manual_seed(0)
    m = MODELS[name]()
    dnn_to_bnn(m, dict(PRIOR, type=typ))
    m = m.to(dev).eval()
    for mod in m.modules():
        if isinstance(mod, nn.modules.batchnorm._BatchNorm):
            mod.to(torch.bfloat16)
    bt.assign_layer_ids(m)
    sites = fuse_model(m) if fuse else 0
    return m, sites


def time_model(name, typ, bs, lanes, replays, fuse):
    import bayesian_torch_amd as bt
    from bayesian_torch_amd import mc
    dev = torch.device("cuda:0")
    m, sites = build(name, typ, dev, fuse)
    x = torch.randn(bs, 3, 224, 224, device=dev).to(torch.bfloat16)
    bt.set_precision("bf16")
    g = mc.GraphedMC(m, x, kl=0.0, lanes=lanes)
    try:
        for k in range(2):  # warm replays
            g.run_many(list(range(k * lanes, (k + 1) * lanes)))
        torch.cuda.synchronize(dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for k in range(replays):
            g.run_many(list(range((k + 2) * lanes, (k + 3) * lanes)))
        e1.record()
        torch.cuda.synchronize(dev)
        ms = e0.elapsed_time(e1) / (replays * lanes)
    finally:
        g.close()
        bt.set_precision("f32")
    return dict(model=name, type=typ, fused=bool(fuse), sites=sites, bs=bs, lanes=lanes, replays=replays,
                ms_per_sample=round(ms, 3))


STORE_LAYERS = [  # (name, kwargs, input) — MobileNetV2 / VGG-shaped layers whose store the activation changes
    ("vgg 3x3 128ch 112^2", dict(in_channels=128, out_channels=128, kernel_size=3, padding=1), (64, 128, 112, 112)),
    ("mbv2 1x1 24->144 56^2", dict(in_channels=24, out_channels=144, kernel_size=1, bias=False), (64, 24, 56, 56)),
    ("mbv2 dw 3x3 144ch 56^2", dict(in_channels=144, out_channels=144, kernel_size=3, padding=1, groups=144, bias=False),
     (64, 144, 56, 56)),
    ("mbv2 1x1 96->576 14^2", dict(in_channels=96, out_channels=576, kernel_size=1, bias=False), (64, 96, 14, 14)),
]


def time_store(typ, reps=20):
    """us per forward_fused launch with the BN folded, ReLU vs ReLU6 (bf16, one MC sample per launch)"""
    from bayesian_torch_amd import layers as L
    dev = torch.device("cuda:0")
    for name, kw, xs in STORE_LAYERS:
        torch.manual_seed(0)
        layer = getattr(L, "Conv2d" + typ)(**kw).to(dev)
        layer.dnn_to_bnn_flag = True
        layer.precision = "bf16"
        x = torch.randn(*xs, device=dev).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
        n = kw["out_channels"]
        scale, shift = torch.rand(n, device=dev) + 0.5, torch.randn(n, device=dev)
        row = dict(layer=name, type=typ)
        with torch.no_grad():
            for act in ("relu", "relu6", "relu", "relu6"):
                for _ in range(3):
                    layer.forward_fused(x, scale, shift, None, act=act)
                torch.cuda.synchronize(dev)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(reps):
                    layer.forward_fused(x, scale, shift, None, act=act)
                e1.record()
                torch.cuda.synchronize(dev)
                row["us_" + act] = round(min(row.get("us_" + act, 1e30), e0.elapsed_time(e1) / reps * 1e3), 1)
        row["relu6_over_relu"] = round(row["us_relu6"] / row["us_relu"], 3)
        print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--type", default="Flipout", choices=["Flipout", "Reparameterization"])
    ap.add_argument("--bs", type=int, default=64)
    ap.add_argument("--lanes", type=int, default=8)
    ap.add_argument("--replays", type=int, default=6)
    ap.add_argument("--models", default="vgg16_bn,mobilenet_v2")
    ap.add_argument("--store", action="store_true", help="also time single layers' fused launches, ReLU vs ReLU6")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("fuse_model_bench needs a GPU")
    if a.store:
        time_store(a.type)
    for name in a.models.split(","):
        row = {}
        for fuse in (False, True):
            t0 = time.perf_counter()
            r = time_model(name, a.type, a.bs, a.lanes, a.replays, fuse)
            r["wall_s"] = round(time.perf_counter() - t0, 1)
            print(json.dumps(r), flush=True)
            row[fuse] = r["ms_per_sample"]
        print(json.dumps(dict(model=name, fused_over_unfused=round(row[True] / row[False], 3))), flush=True)


if __name__ == "__main__":
    main()

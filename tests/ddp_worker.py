"""One rank of tests/test_gpu_ddp.py's two-GPU run, and the small model both sides build.

    python ddp_worker.py RANK WORLD PORT OUT_FILE STEPS

Rank r takes GPU r, joins an RCCL group, runs STEPS replays of GraphedTrainStep(..., optimizer=Adam, group=WORLD) on its shard of the
global batch and leaves its parameters in OUT_FILE."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRIOR = dict(prior_mu=0.0, prior_sigma=1.0, posterior_mu_init=0.0, posterior_rho_init=-3.0, moped_enable=False, moped_delta=0.5)
LOCAL_BS = 4
ADAM = dict(lr=1e-2, weight_decay=1e-3)


def build_small(dev, bn=False):
    """conv(3->8, 3x3) - [BatchNorm] - ReLU - conv(8->8, stride 2) - ReLU - Flatten - Linear(72->5) as Flipout layers, training mode"""
    import bayesian_torch_amd as bt
    bt.manual_seed(9)
    bt.set_precision("f32")
    torch.manual_seed(0)
    mods = [torch.nn.Conv2d(3, 8, 3, padding=1, bias=not bn)] + ([torch.nn.BatchNorm2d(8)] if bn else []) + \
        [torch.nn.ReLU(), torch.nn.Conv2d(8, 8, 3, stride=2), torch.nn.ReLU(), torch.nn.Flatten(), torch.nn.Linear(8 * 3 * 3, 5)]
    net = torch.nn.Sequential(*mods)
    bt.dnn_to_bnn(net, dict(PRIOR, type="Flipout"))
    net = net.to(dev).train()
    bt.assign_layer_ids(net)
    return net


def shard(rank, world, dev):
    g = torch.Generator().manual_seed(5)
    x = torch.randn(world * LOCAL_BS, 3, 8, 8, generator=g)
    y = torch.randint(0, 5, (world * LOCAL_BS,), generator=g)
    return x[rank * LOCAL_BS:(rank + 1) * LOCAL_BS].to(dev), y[rank * LOCAL_BS:(rank + 1) * LOCAL_BS].to(dev)


def main():
    rank, world, port, out, steps = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4], int(sys.argv[5])
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    from bayesian_torch_amd import optim
    from bayesian_torch_amd.autograd import GraphedTrainStep
    dev = torch.device("cuda:%d" % rank)
    torch.cuda.set_device(dev)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
    try:
        net = build_small(dev)
        if rank != 0:  # the broadcast of the construction must bring rank 0's start
            with torch.no_grad():
                for p in net.parameters():
                    p.add_(0.25)
        x, y = shard(rank, world, dev)
        opt = optim.Adam(net.parameters(), max_grad_norm=1.0, **ADAM)
        gs = GraphedTrainStep(net, x, y, optimizer=opt, group=dist.group.WORLD)
        losses = [float(gs.run(s)) for s in range(steps)]
        torch.cuda.synchronize(dev)
        gs.close()
        torch.save({"params": [p.detach().cpu() for p in net.parameters()], "losses": losses}, out)
    finally:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()

"""Data-parallel training: every gradient of a step in ONE flat f32 bucket, ONE all-reduce per step.

What the reference does with DataParallel and a DistributedSampler (examples/main_bayesian_imagenet.py,
main_bayesian_flipout_imagenet.py) becomes, with one process per GPU:

    red = parallel.GradReducer(model)                      # rank 0's parameters and buffers are broadcast
    B = red.global_batch(x.shape[0])
    for step, (x, y) in enumerate(loader):                 # this rank's shard of the global batch
        set_sample_index(model, red.sample_index(step))    # ranks draw independent noise
        loss = ce(model(x), y) + get_kl_loss(model) / B
        loss.backward()
        mean_loss = red.reduce(loss)                       # p.grad is now the mean over the ranks
        optimizer.step(); optimizer.zero_grad()

reduce() is pack -> all_reduce(SUM) -> unpack.  pack multiplies every gradient element (and the loss) by f32(1 / world) into the
bucket, so after the SUM the bucket holds the mean: each rank's loss being CE(local shard) + KL / B_global, the mean over the ranks
is the reference's loss on the global batch.  For a world size that is a power of two the multiply is exact and the result equals
sum-then-divide bit for bit; for any other world size it differs from sum-then-divide by one rounding per element (the products
are rounded before they are added).

Bucket layout: the parameters in model.parameters() order, every offset rounded up to a multiple of 4 floats (tensors that are 16-byte
aligned keep the 16-byte path of the kernels), pad words zeroed at allocation and never written, and ONE last word for the loss.
A parameter's slice is in the parameter's STORAGE order (`grad_view(p)` has p's shape and strides).

On the GPU pack / unpack are the two launches of csrc/btx_bucket.hip (K14: capturable, autograd.GraphedTrainStep(group=) records
them); CPU tensors run the same arithmetic with torch ops, so a gloo group works.  Sample indices: rank r of R uses
(step * R + r) * num_mc + k for pass k of step `step` — distinct indices, hence independent noise, as independent processes of the
reference draw it; the result DOES depend on the number of ranks.  BatchNorm statistics stay local to each rank: sync_buffers()
before an evaluation or a checkpoint."""
import numpy as np
import torch
import torch.distributed as dist

from . import _lib
from ._lib import BtxError
from .optim import _dense

__all__ = ["GradReducer"]


def _flat(t):
    """the n elements of a dense tensor in storage order, as a 1-d view"""
    return t.as_strided((t.numel(),), (1,), t.storage_offset())


class GradReducer:
    def __init__(self, model, group=None, rank=None, world=None, broadcast=True):
        """group: a process group, or None for the default one (no group at all when torch.distributed is not initialised: then
        all_reduce() does nothing).  rank / world override the group's (a test that plays several ranks in one process); the
        collective runs only when `world` is the group's own size.  broadcast: parameters and buffers of rank 0 are copied to
        every rank, in place, and their versions bumped (caches keyed on _version, such as fuse_model's folded BatchNorm, refresh)."""
        live = dist.is_available() and dist.is_initialized()
        r0, w0 = (dist.get_rank(group), dist.get_world_size(group)) if live else (0, 1)
        self.group = group
        self.rank = r0 if rank is None else int(rank)
        self.world = w0 if world is None else int(world)
        if self.world < 1 or not 0 <= self.rank < self.world:
            raise ValueError("rank %d / world %d" % (self.rank, self.world))
        self._live = live and self.world == w0
        self.model = model
        self.scale = float(np.float32(1.0 / self.world))
        self.params = [p for p in model.parameters() if p.requires_grad and p.numel() > 0]
        if not self.params:
            raise ValueError("GradReducer: the model has no parameter that requires a gradient")
        dev = self.params[0].device
        self._offset, off = {}, 0
        for p in self.params:
            if p.device != dev:
                raise BtxError("parameters on more than one device (%s, %s) are not supported" % (dev, p.device))
            if p.dtype != torch.float32 or not _dense(p):
                raise BtxError("the gradient bucket needs float32, non-overlapping and dense parameters: got %s, shape %s, strides %s"
                               % (p.dtype, tuple(p.shape), tuple(p.stride())))
            self._offset[p] = off
            off = (off + p.numel() + 3) & ~3
        self._loss_off = off
        self.bucket = torch.zeros(off + 1, dtype=torch.float32, device=dev)
        self._stage = {}
        self._scale_t = torch.tensor(self.scale, dtype=torch.float32)
        if broadcast and self._live:
            self._broadcast(list(model.parameters()) + list(model.buffers()))

    # ---- conventions ---------------------------------------------------------------------------------------------------
    def sample_index(self, step, k=0, num_mc=1):
        """the MC sample index of pass k of `num_mc` in step `step` on this rank"""
        return ((int(step) * self.world + self.rank) * int(num_mc) + int(k)) & 0x7FFFFFFF

    def global_batch(self, local_bs):
        """the batch the KL term is divided by: local_bs * world"""
        return int(local_bs) * self.world

    @property
    def loss(self):
        """the bucket's last word, 0-d: after reduce() the mean of the ranks' losses"""
        return self.bucket[self._loss_off]

    def grad_view(self, p):
        """the slice of the bucket that belongs to parameter p, with p's shape and strides (after all_reduce(): the mean gradient)"""
        return self.bucket.as_strided(p.shape, p.stride(), self._offset[p])

    # ---- broadcast -------------------------------------------------------------------------------------------------------
    def _broadcast(self, tensors):
        src = 0 if self.group is None else dist.get_global_rank(self.group, 0)
        with torch.no_grad():
            for t in tensors:
                t = t.detach()
                if _dense(t):  # in storage order: a GEMM-major conv parameter is a permuted view, the backends want contiguous
                    dist.broadcast(_flat(t), src=src, group=self.group)
                else:
                    c = t.contiguous()
                    dist.broadcast(c, src=src, group=self.group)
                    t.copy_(c)
        if tensors:
            torch.autograd.graph.increment_version(tensors)

    def sync_buffers(self):
        """broadcast rank 0's buffers (BatchNorm running statistics stay local per rank during training)"""
        if self._live:
            self._broadcast(list(self.model.buffers()))

    # ---- the three phases of reduce() -------------------------------------------------------------------------------------
    def _staged(self, p, g):
        """g in p's storage order: g itself, or p's staging tensor (torch.empty_like(p), as optim._plan does)"""
        if g.stride() == p.stride() or p.numel() == 1:
            return g
        st = self._stage.get(p)
        if st is None:
            st = self._stage[p] = torch.empty_like(p)
        return st

    def _check_grad(self, p, g):
        if g.is_sparse:
            raise BtxError("sparse gradients are not supported (parameter of shape %s)" % (tuple(p.shape),))
        if g.dtype != torch.float32 or g.device != p.device:
            raise BtxError("the gradient of a float32 parameter must be float32 on the same device (got %s on %s, shape %s)"
                           % (g.dtype, g.device, tuple(p.shape)))

    def _items(self, entries):
        items = (_lib.BucketItem * len(entries))()
        for it, (t, off) in zip(items, entries):
            it.src, it.offset, it.n = t.data_ptr(), off, t.numel()
        return items

    @torch.no_grad()
    def pack(self, loss=None):
        """bucket[slice of p] = p.grad * f32(1 / world) for every parameter that has a gradient (a slice whose parameter has none is
        zeroed), bucket[-1] = loss * f32(1 / world).  Capturable on the GPU."""
        entries = []
        for p in self.params:
            g = p.grad
            off = self._offset[p]
            if g is None:
                self.bucket[off:off + p.numel()].zero_()
                continue
            self._check_grad(p, g)
            s = self._staged(p, g)
            if s is not g:
                s.copy_(g)
            entries.append((s, off))
        if loss is not None:
            loss = loss.detach()
            if loss.numel() != 1:
                raise ValueError("loss must hold one element")
            if loss.dtype != torch.float32 or loss.device != self.bucket.device:
                loss = loss.to(device=self.bucket.device, dtype=torch.float32)
            entries.append((loss.reshape(1), self._loss_off))
        if self.bucket.is_cuda:
            # (the item table travels by value in the kernel arguments: nothing of it has to outlive the call)
            _lib.check(_lib.lib().btx_bucket_pack(self._items(entries), len(entries), self.scale, self.bucket.data_ptr(),
                                                  torch.cuda.current_stream(self.bucket.device).cuda_stream))
        else:
            for t, off in entries:
                torch.mul(_flat(t), self._scale_t, out=self.bucket[off:off + t.numel()])
        return self.bucket

    def all_reduce(self):
        """ONE all_reduce(SUM) of the whole bucket, loss word included — also in a 1-rank group, as mc.mc_forward does"""
        if self._live:
            dist.all_reduce(self.bucket, op=dist.ReduceOp.SUM, group=self.group)
        return self.bucket

    @torch.no_grad()
    def unpack(self):
        """p.grad = its slice of the bucket, for every parameter that has a gradient.  Capturable on the GPU."""
        entries, restage = [], []
        for p in self.params:
            g = p.grad
            if g is None:
                continue
            self._check_grad(p, g)
            s = self._staged(p, g)
            if s is not g:
                restage.append((g, s))
            entries.append((s, self._offset[p]))
        if self.bucket.is_cuda:
            _lib.check(_lib.lib().btx_bucket_unpack(self._items(entries), len(entries), self.bucket.data_ptr(),
                                                    torch.cuda.current_stream(self.bucket.device).cuda_stream))
        else:
            for t, off in entries:
                _flat(t).copy_(self.bucket[off:off + t.numel()])
        for g, s in restage:
            g.copy_(s)
        torch.autograd.graph.increment_version([g for g, _ in restage] + [t for t, _ in entries])  # written through raw pointers
        return self.bucket

    def reduce(self, loss=None):
        """pack(loss), all_reduce(), unpack(); returns the mean loss (a 0-d view of the bucket's last word)"""
        self.pack(loss)
        self.all_reduce()
        self.unpack()
        return self.loss

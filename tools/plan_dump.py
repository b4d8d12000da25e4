"""Every plan of the host planner (csrc/btx_plan.cpp) over the sweep of tests/test_plan_invariance.py, one text line per case — no GPU:
  python tools/plan_dump.py > new.txt     BTX_LIB=/other/build/libbtx.so python tools/plan_dump.py > old.txt     diff old.txt new.txt
A tuning change shows with it exactly which plans it moved; a refactor of the planner must leave the dump byte-identical."""
import ctypes
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from bayesian_torch_amd import _lib
import test_plan_invariance as T

L = _lib.lib()
plan = T._Planner()
g, info = plan.g, plan.info
FLAG_VARIANTS = (("gather", _lib.FLAG_GATHER), ("out_f32", _lib.FLAG_OUT_F32), ("out_bf16", _lib.FLAG_OUT_BF16), ("swap_signs", _lib.FLAG_SWAP_SIGNS))


def walk(layers, batches, extra=0, tag=""):
    for name, geo, flags, pool in layers:
        for nb in batches:
            plan.set(geo, nb)
            for kname, kind in T.KINDS:
                for pname, prec, act in T.PRECS:
                    for what, fl, n in [("latency", 0, 1), ("concurrent", _lib.FLAG_CONCURRENT, 1)] + [("lanes=%d" % n, 0, n) for n in T.LANES]:
                        fl |= flags | extra | (n << _lib.FLAG_LANES_SHIFT if n > 1 else 0)
                        rc = L.btx_contract_plan_info(kind, ctypes.byref(g), act, prec, fl, ctypes.byref(plan.pool) if pool else None,
                                                      ctypes.byref(info))
                        hq, wq = ctypes.c_int32(0), ctypes.c_int32(0)
                        ps = L.btx_contract_pool_shape(ctypes.byref(g), act, prec, fl, ctypes.byref(hq), ctypes.byref(wq))
                        print("%s%s nb=%d %s %s %s: rc=%d %s ws=%d sampled_w=%d pool_shape=%d,%d,%d" % (
                            name, tag, nb, kname, pname, what, rc, " ".join("%s=%d" % (f, getattr(info, f)) for f, _ in info._fields_),
                            L.btx_contract_workspace_bytes(ctypes.byref(g), kind, act, prec, fl),
                            L.btx_sampled_w_bytes_lanes(ctypes.byref(g), kind, prec, n), ps, hq.value, wq.value))


walk(T.resnet_layers(), T.BATCHES)
walk(T.other_layers(), (1, 2, 8, 32, 128))
r18 = [l for l in T.resnet_layers() if l[0].startswith(("r18", "stem"))]
for vname, vflag in FLAG_VARIANTS:
    walk(r18, T.BATCHES, vflag, " +" + vname)

"""The backward of BTX-LRT v1 (DESIGN.md §21 "Backward") as a float64 model with the operand roundings of btx_lrt_bwd, and the
per-element bound of every gradient.  Plain module, like lrt_model.py; the contractions run as float64 torch ops on the CPU.

DEFINITION     g = dL/dy,  r = sqrt(v + sigma_b^2) as the forward formed it,  zeta the forward's draw
    c     = r > 0 ? zeta / (2 r) : 0                  (value 0 and gradient DEFINED as 0 at v == 0: the composite's _lrt_root)
    gv    = g c
    dmu   = corr(x, g)          dS   = corr(x^2, gv)          drho   = dS   2 sigma   sigmoid(rho)
    dmu_b = sum_p g             dS_b = sum_p gv               drho_b = dS_b 2 sigma_b sigmoid(rho_b)
    dx    = op^T(g, mu) + 2 x (.) op^T(gv, sigma^2)

OPERANDS (what the library fixed; `act` is the activation dtype, `prec` the layer's precision)
    r          the model takes sqrt(v64) of lrt_model.forward (the FORWARD's operands: lrt_model.operands); the kernel's saved f32 root
               is within c_r = lrt_model.constants(prec, K)[1] of it (relative) — the forward envelope's c_v.
    gv         formed in f32 — 2 r exact, one division, one product — and rounded ONCE to the activation dtype; the weight gradient,
               the bias sum and the data gradient all read that tensor.
               e_gv = (c_r + 4 * 2^-24)(1 + u_act) + u_act      relative error of the stored gv against the model's unrounded g c64
               (c_r for r, 4 * 2^-24 for the division (counted twice: it need not be correctly rounded), the product and, for an f32
               store, its rounding; u_act = 2^-8 for a bf16 store, 0 for f32).
    x^2        x2 = act(f32(x) f32(x)), written once by a HIP launch: the model reproduces it bit for bit.
    weight gradients   exact-f32 MFMA on (x, g) and (x2, gv), partial sums added in a fixed order: accumulation only,
               cw = (K_w + 8) 2^-23 with K_w = batch x output pixels (tests/test_gpu_lrt.py, above _TrainNet).
    factor     2 sigma sigmoid(rho) in f32: softplus within envelope.DELTA_W, expf, one division, three products:
               e_fac = DELTA_W + 8 * 2^-24 (the 8 * 2^-24 of tests/test_gpu_lrt.py).
    data gradient      two noise-free contractions in precision `prec`, f32 accumulation: cd = (K_d + 8) 2^-23, K_d = taps x output
               channels.  prec f32: operands g, mu, gv, f32(sigma^2) — sigma^2 within op_s = 2 DELTA_W + 2^-24 of the model's.
               prec bf16: g and gv enter as bf16 (an f32 activation is rounded in staging: the model reproduces bf16(g); gv takes
               one more u on top of e_gv), mu as bf16(mu) (reproduced), sigma^2 as bf16(f32(sigma^2)) — within
               op_s = (2u + 2 DELTA_W + 2^-24)(1 + u) of the model's bf16(sigma^2), as in the forward (lrt_model.py).
               A = op^T(g, mu) and B = op^T(gv, sigma^2) are each stored in the activation dtype (u_act each), then
               dx = act(fma(2 x, B, A)): one f32 rounding and the store's.

BOUNDS         with A_* the same contraction on absolute values (envelope.wgrad_A / dgrad_A) and u32 = 2^-24
    dmu        cw A_mu + u32 |ref|
    drho       (cw + e_gv + e_fac)(1 + e_gv) A_s2 fac + u32 |ref|           A_s2 = corr(x2, |gv|),  fac = 2 sigma sigmoid(rho)
    dmu_b      cw sum|g| + u32 |ref|
    drho_b     (cw + e_gv + e_fac)(1 + e_gv) sum|gv| fac_b + u32 |ref|
    dx         bA = cd A_1,  bB = (cd + e_gv' + op_s)(1 + e_gv') A_2        A_1 = op^T(|g|, |mu|), A_2 = op^T(|gv|, sigma^2)
               b  = bA + u_act (|A| + bA) + 2 |x| (bB + u_act (|B| + bB));  dx: b + (u32 + u_act)(|ref| + b)
Where a bound is 0 the value must be 0 exactly (v == 0 everywhere: drho, drho_b and the B term of dx).

A missing factor 2 in dx, a zeta shifted by one index, a dropped sigma_b^2 under the root and a removed v == 0 guard all land far
outside: they change a gradient by a quantity of the order of its noise part against bounds that are ~2^-8 (bf16) or ~1e-5 (f32)
of the same magnitudes (tests/test_lrt_train_cpu.py pins this with perturbed references).
"""
import numpy as np
import torch

import envelope as E
import lrt_model as LM

U = E.U_BF16
U32 = 2.0 ** -24


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64)))


def _dgrad64(dy, x_shape, w, op):
    """op^T(dy, w) in float64: autograd through the float64 contraction"""
    xz = torch.zeros(x_shape, dtype=torch.float64, requires_grad=True)
    (g,) = torch.autograd.grad(E.contract(xz, w, None, op), xz, dy)
    return g


def _chan_axis(ndim):
    return 1 if ndim > 2 else ndim - 1


def constants(prec, act_bf16, Kf, Kw, Kd, delta_w=E.DELTA_W):
    """-> dict(c_r, e_gv, e_gvx, e_fac, op_s, cw, cd, u_act)"""
    u_act = U if act_bf16 else 0.0
    c_r = LM.constants(prec, Kf, False, delta_w)[1]
    e_gv = (c_r + 4 * U32) * (1 + u_act) + u_act
    e_gvx = e_gv + (U * (1 + e_gv) if (prec == "bf16" and not act_bf16) else 0.0)  # an f32 gv rounded to bf16 in staging
    op_s = 2 * delta_w + U32 if prec == "f32" else (2 * U + 2 * delta_w + U32) * (1 + U)
    return dict(c_r=c_r, e_gv=e_gv, e_gvx=e_gvx, e_fac=delta_w + 8 * U32, op_s=op_s, cw=(Kw + 8) * E.ACC_UNIT,
                cd=(Kd + 8) * E.ACC_UNIT, u_act=u_act)


def backward(x, g, zeta, mu, rho, mu_b, rho_b, op, prec="f32", act_bf16=False, exact=False, dx_factor=2.0, drop_bias_var=False,
             guard=True):
    """float64 gradients of one layer and their bounds.  x, g: float32 arrays holding activation-dtype values, logical layouts; zeta in
    the output's logical shape; mu, rho (, mu_b, rho_b) float32 logical.  exact=True: no operand rounding at all (the semantic
    definition: equals float64 autograd of the composite).  dx_factor / drop_bias_var / guard: the perturbed references of the tests.
    -> dict(ref={mu, rho, mu_b, rho_b, x}, bound={...}, root, gv, K=(Kf, Kw, Kd))"""
    x = np.asarray(x, dtype=np.float32)
    g = np.asarray(g, dtype=np.float32)
    mu = np.asarray(mu, dtype=np.float32)
    z = _t(zeta)
    wshape = tuple(mu.shape)
    has_b = mu_b is not None
    if exact:
        sg = np.log1p(np.exp(np.asarray(rho, dtype=np.float64)))
        x64, x2f, x2b, s2f, s2b, mu_d, g_d = _t(x), _t(x) ** 2, _t(x) ** 2, _t(sg * sg), _t(sg * sg), _t(mu), _t(g)
        sb = np.log1p(np.exp(np.asarray(rho_b, dtype=np.float64))) if has_b else None
    else:
        xr, x2fw, mu_r, s2 = LM.operands(x, mu, rho, prec)          # the forward's operands: they define r
        x64, x2f, s2f = _t(x), _t(x2fw), _t(s2)
        x2a = (x * x).astype(np.float32)                             # the backward's x2 = act(x * x)
        x2b = _t(LM.rbf16(x2a) if act_bf16 else x2a)
        s2b, mu_d = _t(s2), _t(mu_r)                                 # data gradient: the precision's operands
        g_d = _t(LM.rbf16(g) if prec == "bf16" else g)
        sg = LM.sigma32(rho).astype(np.float64)
        sb = LM.sigma32(rho_b).astype(np.float64) if has_b else None
    vb = _t(sb * sb) if (has_b and not drop_bias_var) else None
    v = E.contract(x2f, s2f, vb, op)
    g64 = _t(g)
    if guard:
        pos = v > 0
        r = torch.where(pos, torch.sqrt(torch.where(pos, v, torch.ones_like(v))), torch.zeros_like(v))
        c = torch.where(pos, z / (2.0 * torch.where(pos, r, torch.ones_like(r))), torch.zeros_like(v))
    else:
        r = torch.sqrt(v)
        with np.errstate(all="ignore"):
            c = z / (2.0 * r)
    gv = g64 * c
    fac = _t(2.0 * sg / (1.0 + np.exp(-np.asarray(rho, dtype=np.float64))))
    red = [d for d in range(g64.dim()) if d != _chan_axis(g64.dim())]
    ref = {"mu": E.wgrad64(x64, g64, wshape, op), "rho": E.wgrad64(x2b, gv, wshape, op) * fac}
    A = _dgrad64(g_d, tuple(x.shape), mu_d, op)
    B = _dgrad64(gv, tuple(x.shape), s2b, op)
    ref["x"] = A + dx_factor * x64 * B
    if has_b:
        fac_b = _t(2.0 * sb / (1.0 + np.exp(-np.asarray(rho_b, dtype=np.float64))))
        ref["mu_b"] = g64.sum(red)
        ref["rho_b"] = gv.sum(red) * fac_b
    Kf, Kw, Kd = E.reduction_length(wshape, op), E.wgrad_reduction_length(tuple(g.shape), op), E.dgrad_reduction_length(wshape, op)
    k = constants(prec, act_bf16, Kf, Kw, Kd)
    gva = torch.nan_to_num(gv.abs(), nan=0.0, posinf=0.0, neginf=0.0)
    e1 = (k["cw"] + k["e_gv"] + k["e_fac"]) * (1 + k["e_gv"])
    bnd = {"mu": k["cw"] * E.wgrad_A(x64, g64, wshape, op), "rho": e1 * E.wgrad_A(x2b, gva, wshape, op) * fac}
    bA = k["cd"] * E.dgrad_A(g_d, tuple(x.shape), mu_d.abs(), op)
    bB = (k["cd"] + k["e_gvx"] + k["op_s"]) * (1 + k["e_gvx"]) * E.dgrad_A(gva, tuple(x.shape), s2b, op)
    ua = k["u_act"]
    bx = bA + ua * (A.abs() + bA) + 2.0 * x64.abs() * (bB + ua * (torch.nan_to_num(B.abs(), nan=0.0) + bB))
    bnd["x"] = bx
    if has_b:
        bnd["mu_b"] = k["cw"] * g64.abs().sum(red)
        bnd["rho_b"] = e1 * gva.sum(red) * fac_b
    out_b = {}
    for q, b in bnd.items():
        b, rf = b.numpy(), np.nan_to_num(np.abs(ref[q].numpy()), nan=0.0, posinf=0.0)
        out_b[q] = b + ((U32 + ua) * (rf + b) if q == "x" else U32 * rf)
    return dict(ref={q: t.numpy() for q, t in ref.items()}, bound=out_b, root=r.numpy(), gv=gv.numpy(), K=(Kf, Kw, Kd), c_r=k["c_r"])


def composite_autograd64(x, g, zeta, mu, rho, mu_b, rho_b, op):
    """torch float64 autograd of the composite (base_variational_layer._lrt_composite with its _lrt_root guard) -> {name: grad}"""
    P = {"mu": _t(mu).requires_grad_(), "rho": _t(rho).requires_grad_()}
    if mu_b is not None:
        P["mu_b"], P["rho_b"] = _t(mu_b).requires_grad_(), _t(rho_b).requires_grad_()
    x64 = _t(x).requires_grad_()
    sg = torch.log1p(torch.exp(P["rho"]))
    mb = vb = None
    if mu_b is not None:
        sb = torch.log1p(torch.exp(P["rho_b"]))
        mb, vb = P["mu_b"], sb * sb
    m = E.contract(x64, P["mu"], mb, op)
    v = E.contract(x64 * x64, sg * sg, vb, op)
    pos = v > 0
    root = torch.where(pos, torch.sqrt(torch.where(pos, v, torch.ones_like(v))), torch.zeros_like(v))
    (m + root * _t(zeta)).backward(_t(g))
    out = {q: t.grad.numpy() for q, t in P.items()}
    out["x"] = x64.grad.numpy()
    return out

"""numpy model of BTX-EVAL v1: the evaluation head of the packed MC statistics, mc.Evaluator.

The model IS the definition: the CPU path of mc.Evaluator equals it bit for bit, the kernel (csrc/btx_mceval.hip) equals it in
every integer decision and in conf / p_y, and differs in the values that go through logf only by what `reference64` bounds
(the model's logf is the correctly rounded one, log in float64 rounded to f32; the device's is its math library's).

Record of a row (8 floats): pred, rank, conf, p_y, nll, brier, H, MI.
State (float64): see STATE_* below, then bins[nbins][count, sum conf, hits], then quad[T][n_ac, n_au, n_ic, n_iu].
"""
import numpy as np

EPS = np.float32(1e-15)
ROW_THREADS = 256
HEADER, CURSOR, DROPPED = 16, 11, 12
S_VALID, S_IGNORED, S_TOP1, S_TOPK, S_NLL, S_BRIER, S_H, S_MI, S_CONF, S_U_CORRECT, S_U_INCORRECT = range(11)
REC_PRED, REC_RANK, REC_CONF, REC_PY, REC_NLL, REC_BRIER, REC_H, REC_MI = range(8)

C0_ULP = 3.77  # envelope.C0_ULP: the device's expf / logf against float64, in ulps (profiles/reduction_envelope.txt)
U32 = 2.0 ** -24
U64 = 2.0 ** -53
TINY32 = 2.0 ** -149


def packed_numel(bs, C):
    return 2 * bs * C + bs + 2


def pack_probs(probs):
    """probs [S, bs, C] float32 -> the packed vector mc.accumulate builds, sample by sample, in f32"""
    S, bs, C = probs.shape
    p = probs.astype(np.float32)
    out = np.zeros(packed_numel(bs, C), np.float32)
    for s in range(S):
        out[:bs * C] += p[s].reshape(-1)
        out[bs * C:2 * bs * C] += (p[s] * p[s]).reshape(-1)
        out[2 * bs * C:2 * bs * C + bs] += -row_sum(p[s] * logf(p[s] + EPS))
        out[-1] += np.float32(1)
    return out


def logf(x):
    """the model's logf: correctly rounded (float64 log, rounded once)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.log(np.asarray(x, np.float32).astype(np.float64)).astype(np.float32)


def row_sum(terms):
    """f32 sum over the last axis in the kernel's shape: thread t adds c = t, t + 256, ... in order, a butterfly inside each of
    the four waves, then (w0 + w1) + (w2 + w3)"""
    terms = np.asarray(terms, np.float32)
    C = terms.shape[-1]
    k = -(-C // ROW_THREADS)
    pad = np.zeros(terms.shape[:-1] + (k * ROW_THREADS,), np.float32)
    pad[..., :C] = terms
    w = pad.reshape(terms.shape[:-1] + (k, ROW_THREADS))
    acc = np.zeros(terms.shape[:-1] + (ROW_THREADS,), np.float32)
    for j in range(k):
        acc = acc + w[..., j, :]
    acc = acc.reshape(terms.shape[:-1] + (4, 64))
    for off in (32, 16, 8, 4, 2, 1):
        acc = acc[..., :off] + acc[..., off:2 * off]
    acc = acc[..., 0]
    return (acc[..., 0] + acc[..., 1]) + (acc[..., 2] + acc[..., 3])


def fold_sum(v):
    """float64 sum over the last axis (the rows of a batch) in the fold's shape: lane l adds rows l, l + 64, ... in order, then a
    butterfly over the 64 lanes"""
    v = np.asarray(v, np.float64)
    n = v.shape[-1]
    k = -(-n // 64)
    pad = np.zeros(v.shape[:-1] + (k * 64,), np.float64)
    pad[..., :n] = v
    w = pad.reshape(v.shape[:-1] + (k, 64))
    acc = np.zeros(v.shape[:-1] + (64,), np.float64)
    for j in range(k):
        acc = acc + w[..., j, :]
    for off in (32, 16, 8, 4, 2, 1):
        acc = acc[..., :off] + acc[..., off:2 * off]
    return acc[..., 0]


def split(packed, bs, C):
    packed = np.asarray(packed, np.float32)
    return (packed[:bs * C].reshape(bs, C), packed[2 * bs * C:2 * bs * C + bs], packed[2 * bs * C + bs + 1])


def rows(packed, labels, bs, C):
    """-> records [bs, 8] float32"""
    sum_p, sum_h, n = split(packed, bs, C)
    y = np.asarray(labels, np.int64).reshape(bs)
    valid = (y >= 0) & (y < C)
    yi = np.where(valid, y, -1)
    p = sum_p / n  # f32 / f32
    pred = p.argmax(1)  # numpy: the first of equal maxima
    conf = p[np.arange(bs), pred]
    py = np.where(valid, p[np.arange(bs), np.where(valid, y, 0)], np.float32(0)).astype(np.float32)
    c = np.arange(C)[None, :]
    rank = ((p > py[:, None]) | ((p == py[:, None]) & (c < yi[:, None]))).sum(1)
    H = -row_sum(p * logf(p + EPS))
    d = p - (c == yi[:, None]).astype(np.float32)
    brier = row_sum(d * d)
    MI = H - sum_h / n
    rec = np.zeros((bs, 8), np.float32)
    rec[:, REC_PRED] = pred
    rec[:, REC_RANK] = np.where(valid, rank, -1)
    rec[:, REC_CONF] = conf
    rec[:, REC_PY] = py
    rec[:, REC_NLL] = np.where(valid, -logf(py + EPS), np.float32(0))
    rec[:, REC_BRIER] = np.where(valid, brier, np.float32(0))
    rec[:, REC_H] = H
    rec[:, REC_MI] = MI
    return rec


def bin_index(conf, nbins):
    e = np.ceil(np.asarray(conf, np.float32) * np.float32(nbins))
    return np.clip(e.astype(np.int64) - 1, 0, nbins - 1)


def state_doubles(nbins, T):
    return HEADER + 3 * nbins + 4 * T


def new_state(nbins=15, T=0):
    return np.zeros(state_doubles(nbins, T), np.float64)


def fold(state, rec, topk=5, nbins=15, th=(), use_mi=False, capacity=0):
    """state += the batch whose records are rec [bs, 8] (in place)"""
    bs = rec.shape[0]
    th = np.asarray(th, np.float32).reshape(-1)
    T = th.size
    rank = rec[:, REC_RANK]
    valid, hit = rank >= 0, rank == 0
    u32 = rec[:, REC_MI] if use_mi else rec[:, REC_H]
    u = u32.astype(np.float64)
    z = np.zeros(bs)
    q = np.zeros((11 + 3 * nbins + 4 * T, bs), np.float64)
    q[S_VALID] = valid
    q[S_IGNORED] = ~valid
    q[S_TOP1] = hit
    q[S_TOPK] = valid & (rank < np.float32(topk))
    for j, col in ((S_NLL, REC_NLL), (S_BRIER, REC_BRIER), (S_H, REC_H), (S_MI, REC_MI), (S_CONF, REC_CONF)):
        q[j] = np.where(valid, rec[:, col].astype(np.float64), z)
    q[S_U_CORRECT] = np.where(hit, u, z)
    q[S_U_INCORRECT] = np.where(valid & ~hit, u, z)
    b = bin_index(rec[:, REC_CONF], nbins)
    for k in range(nbins):
        m = valid & (b == k)
        q[11 + 3 * k] = m
        q[11 + 3 * k + 1] = np.where(m, rec[:, REC_CONF].astype(np.float64), z)
        q[11 + 3 * k + 2] = m & hit
    for t in range(T):
        cert = u32 <= th[t]
        q[11 + 3 * nbins + 4 * t + 0] = valid & hit & cert
        q[11 + 3 * nbins + 4 * t + 1] = valid & hit & ~cert
        q[11 + 3 * nbins + 4 * t + 2] = valid & ~hit & cert
        q[11 + 3 * nbins + 4 * t + 3] = valid & ~hit & ~cert
    s = fold_sum(q)
    state[:11] = state[:11] + s[:11]
    state[HEADER:HEADER + 3 * nbins + 4 * T] = state[HEADER:HEADER + 3 * nbins + 4 * T] + s[11:]
    cur = state[CURSOR]
    state[DROPPED] += min(max(cur + bs - capacity, 0.0), float(bs))
    state[CURSOR] = cur + bs
    return state


def update(state, packed, labels, bs, C, topk=5, nbins=15, th=(), use_mi=False, records=None):
    """one Evaluator.update: the records of the batch go to records[cursor ...] (a [capacity, 8] array or None) -> rec"""
    rec = rows(packed, labels, bs, C)
    capacity = 0 if records is None else records.shape[0]
    cur = int(state[CURSOR])
    keep = max(0, min(bs, capacity - cur))
    if keep:
        records[cur:cur + keep] = rec[:keep]
    fold(state, rec, topk, nbins, th, use_mi, capacity)
    return rec


# ---- float64 recomputation and envelopes ----------------------------------------------------------------------------------
def reference64(packed, labels, bs, C, c0=C0_ULP):
    """nll, brier, H, MI of every row in float64 from the SAME packed contents, each with the bound of what an implementation of
    BTX-EVAL v1 may differ by (style of envelope.mc_reference: u = 2^-24 per f32 rounding, c0 ulps for logf, one unit per level of
    a reduction: ceil(C / 256) chain additions + 6 butterfly steps + 2) -> dict name -> (value [bs], bound [bs])"""
    sum_p, sum_h, n = split(packed, bs, C)
    u = U32
    y = np.asarray(labels, np.int64).reshape(bs)
    valid = (y >= 0) & (y < C)
    ys = np.where(valid, y, 0)
    p = sum_p.astype(np.float64) / float(n)
    bp = u * p + TINY32                                  # the f32 division
    a = p + float(EPS)
    L = np.log(a)
    ra = bp / a + u                                      # the f32 addition of the epsilon
    bL = ra / (1 - ra) + c0 * 2.0 ** -23 * np.abs(L) + TINY32
    t = p * L
    bt = bp * (np.abs(L) + bL) + p * bL + u * (np.abs(t) + bp * np.abs(L)) + TINY32
    levels = -(-C // ROW_THREADS) + 8
    H = -t.sum(1)
    bH = bt.sum(1) + levels * u * (np.abs(t) + bt).sum(1)
    q = sum_h.astype(np.float64) / float(n)
    bq = u * np.abs(q) + TINY32
    MI = H - q
    bMI = bH + bq + u * (np.abs(H) + np.abs(q) + bH + bq)
    r = np.arange(bs)
    nll = -L[r, ys]
    bnll = bL[r, ys]
    d = p - (np.arange(C)[None, :] == y[:, None])
    bd = bp + u * np.abs(d)
    d2 = d * d
    bd2 = 2 * np.abs(d) * bd + bd * bd + u * (np.abs(d) + bd) ** 2 + TINY32
    brier = d2.sum(1)
    bbrier = bd2.sum(1) + levels * u * (d2 + bd2).sum(1)
    zero = np.zeros(bs)
    return {"H": (H, bH), "MI": (MI, bMI), "nll": (np.where(valid, nll, zero), np.where(valid, bnll, zero)),
            "brier": (np.where(valid, brier, zero), np.where(valid, bbrier, zero)), "conf": (p.max(1), bp.max(1)), "valid": valid}


def state_sum_bound(values, bounds):
    """bound of a float64 state sum over the rows: the rows' own bounds plus the fold's additions (ceil(bs / 64) + 6 levels, one
    more into the state) at 2^-53"""
    values, bounds = np.asarray(values, np.float64), np.asarray(bounds, np.float64)
    levels = -(-values.size // 64) + 7
    return bounds.sum() + levels * U64 * (np.abs(values) + bounds).sum()


# ---- constructed exact cases -----------------------------------------------------------------------------------------------
def exact_cases():
    """n = 8 samples, sums that are multiples of 2^-7: every p is exact, every integer decision is forced.
    -> list of (name, packed, labels, bs, C, nbins, expected dict)"""
    out = []

    def pk(sum_p, n=8.0):
        sum_p = np.asarray(sum_p, np.float32)
        bs, C = sum_p.shape
        v = np.zeros(packed_numel(bs, C), np.float32)
        v[:bs * C] = sum_p.reshape(-1)
        v[bs * C:2 * bs * C] = (sum_p * sum_p / 8).reshape(-1)
        v[-1] = n
        return v, bs, C
    # two equal maxima: pred is the lower index; a label on the higher one has rank 1, on the lower one rank 0
    sp = np.array([[1, 3, 3, 1], [1, 3, 3, 1], [3, 1, 1, 3]], np.float32)
    v, bs, C = pk(sp)
    out.append(("equal_maxima", v, np.array([2, 1, 3]), bs, C, 15, dict(pred=[1, 1, 0], rank=[1, 0, 1])))
    # ties below and above y: p = [2, 1, 2, 1, 1, 1] / 8; y = 3 -> two larger, one equal below (index 1) -> rank 3
    sp = np.array([[2, 1, 2, 1, 1, 1]] * 4, np.float32)
    v, bs, C = pk(sp)
    out.append(("rank_ties", v, np.array([3, 1, 5, 2]), bs, C, 15, dict(pred=[0] * 4, rank=[3, 2, 5, 1])))
    # uniform C = 16, nbins = 16: conf = 1/16, conf * 16 = 1 exactly -> bin 0 (right-closed)
    sp = np.full((2, 16), 0.5, np.float32)
    v, bs, C = pk(sp)
    out.append(("uniform16", v, np.array([0, 7]), bs, C, 16, dict(pred=[0, 0], rank=[0, 7], bin=[0, 0])))
    # conf = 0.5, nbins = 10: conf * 10 = 5 exactly -> bin 4
    sp = np.array([[4, 2, 2], [2, 4, 2]], np.float32)
    v, bs, C = pk(sp)
    out.append(("half10", v, np.array([0, 0]), bs, C, 10, dict(pred=[0, 1], rank=[0, 1], bin=[4, 4])))
    return out


# ---- the fixture (tests/golden/mc_eval.npz, tools/make_golden_mc_eval.py) ----------------------------------------------------
GOLDEN_CASES = ("s8_b48_c10", "s4_b7_c1000", "s20_b64_c257", "s5_b33_c2")
_CACHE = {}


def golden_case(name):
    """-> dict of the case's arrays plus S, B, C, logits widened to f32, probs (torch's f32 softmax, as the reference's
    evaluate() takes it) and packed (the f32 sums of the probabilities, sample by sample).  Computed once; do not modify."""
    import os
    if name not in _CACHE:
        import torch
        z = _CACHE.get("npz")
        if z is None:
            z = _CACHE["npz"] = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mc_eval.npz"))
        d = {k.split("/", 1)[1]: z[k] for k in z.files if k.startswith(name + "/")}
        d["logits"] = d["logits"].astype(np.float32)
        d["S"], d["B"], d["C"] = d["logits"].shape
        d["probs"] = torch.softmax(torch.from_numpy(d["logits"]), dim=-1).numpy()
        d["packed"] = pack_probs(d["probs"])
        _CACHE[name] = d
    return _CACHE[name]

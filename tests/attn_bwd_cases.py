"""Cases, float64 oracle and error bounds for the attention backward kernels (parq_amd/csrc/attn_bwd.hip), called one launcher at a
time through parq_k_attention_backward / parq_k_attention_backward_batched.  Shared by tests/test_attn_bwd_cpu.py (the oracle against
autograd and central differences, the plan of every case) and tests/test_gpu_attn_bwd.py (the kernels against the oracle).

The oracle is spelled out, not taken from autograd, per (scene, head) and iteration t, in float64:
    S = q k^T / sqrt(dh),  P = softmax(S),  lse2 = log2 sum exp(S),  Pd = P keep / (1 - p)  (keep: the dropout mask; 1 without dropout)
    O = Pd v,  D = rowsum(dO * O),  dP = dO v^T,  dS = P (dP keep / (1 - p) - D)
    dV = sum_t Pd^T dO,  dK = sum_t dS^T q / sqrt(dh),  dQ_t = dS k / sqrt(dh)
Its own O and lse2, rounded to fp32, are what the kernels are given: the backward is judged apart from the forward kernels.

Next to every gradient it returns A, the sum of the absolute values of the terms of its contraction with dS expanded into ITS terms:
    Psi = |dO| |v|^T,  Theta = rowsum|dO * O|,  T = P (Psi keep / (1 - p) + Theta)  >= |dS|
    A_dV = sum_t Pd^T |dO|,  A_dK = sum_t T^T |q| / sqrt(dh),  A_dQ_t = T |k| / sqrt(dh)
dS = P (dP - D) cancels, so its rounding error is relative to T, not to |dS|: a bound alpha * A holds with A built from T only.
A >= |gradient| elementwise.  The sums that the absolute floors of the 16-bit forms need come with it (sT_q, sT_k, sPd_k)."""
import ctypes as C
import math
import zlib

import numpy as np
import torch

U = 2.0 ** -24                       # unit roundoff of fp32
LOG2E = 1.4426950408889634
(FAM_VALU32, FAM_MFMA2, FAM_MFMA8, FAM_SPLIT, FAM_MAT, FAM_SPLIT2, FAM_B256) = range(1, 8)
FAM_NAME = {FAM_VALU32: "valu32", FAM_MFMA2: "mfma2", FAM_MFMA8: "mfma8", FAM_SPLIT: "split", FAM_MAT: "materialised",
            FAM_SPLIT2: "split2", FAM_B256: "batched256"}
SELF, CROSS = 0, 1
F16, BF16 = 0, 1


def _case(name, launcher, dh, B, H, Lq, Lk, n_it, plan, **kw):
    d = dict(name=name, launcher=launcher, dh=dh, B=B, H=H, Lq=Lq, Lk=Lk, n_it=n_it, plan=plan, use_absmax=0)
    d.update(kw)
    return d


def _slots(Lk):
    return -(-Lk // 256)


# plan = (kernel family, key blocks per workgroup, dQ partial slots per (scene, head), QP) as the case table of the issue claims it
CASES = {c["name"]: c for c in [
    _case("g4_whole", "batched", 64, 32, 4, 40, 4096, 2, (FAM_SPLIT2, 4, 4, 0)),       # 16 blocks, every group full, not ragged
    _case("g4_ragged", "batched", 64, 32, 4, 40, 4500, 2, (FAM_SPLIT2, 4, 5, 0)),      # 18 blocks: last group has 2, last block 148 keys
    _case("g2_stage", "batched", 64, 32, 4, 33, 2368, 2, (FAM_SPLIT2, 2, 5, 0)),       # 10 blocks, ragged, whole 64-key stages
    _case("g2_whole", "batched", 64, 32, 4, 32, 2304, 1, (FAM_SPLIT2, 2, 5, 0)),       # 9 blocks: last group has 1; n_it 1
    _case("g1_iters16", "batched", 64, 1, 2, 24, 2049, 16, (FAM_SPLIT2, 1, 9, 0)),     # kMaxBwdIters, one key in the last block
    _case("g1_q1", "batched", 64, 2, 1, 1, 2560, 3, (FAM_SPLIT2, 1, 10, 0)),           # one query: 31 padded rows per tile
    _case("b256_two_slices", "batched", 256, 2, 2, 200, 333, 3, (FAM_B256, 1, 0, 1024)),   # the second 512-row slice, zero rows past 600
    _case("b256_small", "batched", 256, 1, 1, 24, 32, 1, (FAM_B256, 1, 0, 512)),
] + [_case("s32_q%d_k%d" % (Lq, Lk), "single", 32, 2, 2, Lq, Lk, 0, (FAM_VALU32, 1, 0, 0))
     for Lq, Lk in ((1, 1), (33, 255), (33, 256), (33, 257), (33, 600), (1, 600))
] + [_case("s64_short_q%d_k%d" % (Lq, Lk), "single", 64, 2, 2, Lq, Lk, 0, (FAM_MFMA2, 1, 0, 0))
     for Lq, Lk in ((1, 1), (40, 63), (40, 64), (40, 65), (40, 2047), (1, 2047))
] + [_case("s64_long_k%d_%s" % (Lk, "split" if ab else "exact"), "single", 64, 2, 2, 40, Lk, 0,
           (FAM_SPLIT if ab else FAM_MFMA8, 1, _slots(Lk), 0), use_absmax=ab)
     for Lk in (2048, 2049, 2300) for ab in (1, 0)
] + [_case("smat_d%d_k%d" % (dh, Lk), "single", dh, 1, 2, 24, Lk, 0, (FAM_MAT, 1, 0, 0)) for dh in (128, 256) for Lk in (17, 300)]}


def _spec(case, **kw):
    s = dict(case=case, drop=0.0, cache=0, kind=F16, layout=CROSS, acc=0, det=0, do_exp=0, do_zero=0)
    s.update(kw)
    c = CASES[case]
    parts = [case]
    if c["launcher"] == "single":
        parts += ["self" if s["layout"] == SELF else "cross", "acc%d" % s["acc"]]
        if s["det"]:
            parts.append("det")
    if s["drop"]:
        parts.append("p%g" % s["drop"])
    if s["cache"]:
        parts.append("c%d%s" % (s["cache"], "bf" if s["kind"] == BF16 else ""))
    if s["do_exp"]:
        parts.append("dOx2^%+d" % s["do_exp"])
    if s["do_zero"]:
        parts.append("dO0")
    s["id"] = "-".join(parts)
    return s


def specs():
    """Every run of the GPU tier: the rows of the case table with the variants of the issue."""
    out = []
    for name, c in CASES.items():
        if c["launcher"] == "batched":
            out += [_spec(name), _spec(name, drop=0.25)]                       # dropout 0 and 0.25 on every batched row
        else:
            i = list(CASES).index(name)
            for layout in ((SELF, CROSS) if name.startswith("s32") else ((SELF, CROSS)[i % 2],)):
                for acc in (0, 1):                                              # accumulate_kv 0 and 1 on the single rows
                    out.append(_spec(name, layout=layout, acc=acc))
                    if c["plan"][0] == FAM_MFMA2:                               # ... with and without the deterministic scratch
                        out.append(_spec(name, layout=layout, acc=acc, det=1))
    for name in ("s32_q33_k257", "s64_short_q40_k65", "s64_long_k2300_split", "s64_long_k2049_exact", "smat_d128_k300", "smat_d256_k17"):
        out.append(_spec(name, drop=0.25, acc=1))                               # dropout on one row of each single family
    out.append(_spec("s64_short_q40_k2047", drop=0.25, det=1))
    for name, drops in (("g4_ragged", (0.0,)), ("g1_iters16", (0.0, 0.25))):   # cache_terms 3 and 1 (both kinds); 0 is above
        for p in drops:
            out += [_spec(name, drop=p, cache=3), _spec(name, drop=p, cache=1), _spec(name, drop=p, cache=1, kind=BF16)]
    out += [_spec("g2_stage", drop=0.25, cache=8), _spec("g2_whole", cache=8), _spec("g2_whole", drop=0.25, cache=8)]
    for name in ("g2_whole", "s64_long_k2300_split", "s64_long_k2300_exact"):  # the power-of-two gradient scale
        out += [_spec(name, do_exp=-20), _spec(name, do_exp=20), _spec(name, do_zero=1)]
    ids = [s["id"] for s in out]
    assert len(set(ids)) == len(ids)
    return out


# ------------------------------------------------------------------------------------------------ inputs
def seed_of(name):
    return zlib.crc32(name.encode()) & 0x7FFFFFFF


def drop_seeds(case):
    c = CASES[case]
    return [(seed_of(case) * 2654435761 + 7919 * t + 1) & 0xFFFFFFFF for t in range(max(1, c["n_it"]))]


def make_inputs(case):
    """Seeded fp32 inputs: q, dO [T][B][H][Lq][dh], k, v [B][H][Lk][dh] (T = 1 for the single launcher).  Unit normal, except that in
    every (scene, head) the keys Lk // 2 and Lk - 1 are aligned with queries 0 and Lq - 1 of iteration 0 (score ~ 12: P near 1 on those
    rows, near-uniform rows elsewhere).  The last key — the one a ragged last block holds — is one of the peaks."""
    c = CASES[case]
    T, B, H, Lq, Lk, dh = max(1, c["n_it"]), c["B"], c["H"], c["Lq"], c["Lk"], c["dh"]
    g = np.random.Generator(np.random.PCG64(seed_of(case)))
    q = g.standard_normal((T, B, H, Lq, dh), dtype=np.float32)
    dO = g.standard_normal((T, B, H, Lq, dh), dtype=np.float32)
    k = g.standard_normal((B, H, Lk, dh), dtype=np.float32)
    v = g.standard_normal((B, H, Lk, dh), dtype=np.float32)
    s = np.float32(12.0 / math.sqrt(dh))
    k[:, :, Lk // 2] = s * q[0, :, :, 0]
    k[:, :, Lk - 1] = s * q[0, :, :, Lq - 1]
    return dict(q=q, k=k, v=v, dO=dO)


def prefill(shape, salt):
    """Non-zero seeded pre-fill of an output that is added to, or of columns that must stay untouched: |x| in [1, 2) 2^-3."""
    g = np.random.Generator(np.random.PCG64(1000 + salt))
    x = (1.0 + g.random(shape, dtype=np.float32)) * np.float32(0.125)
    return (x * np.where(g.random(shape, dtype=np.float32) < 0.5, np.float32(-1), np.float32(1))).astype(np.float32)


# ------------------------------------------------------------------------------------------------ dropout keep-masks
def _mix(x):
    x = x ^ (x >> np.uint32(16)); x = x * np.uint32(0x7feb352d); x = x ^ (x >> np.uint32(15))
    x = x * np.uint32(0x846ca68b)
    return x ^ (x >> np.uint32(16))


def keep_mask(seed, rows, cols, p):
    """NumPy restatement of drop_keep(drop_rowhash(seed, row), col, p) (parq_amd/csrc/common.hpp) on the (rows, cols) index space, in
    wrapping uint32 arithmetic: the same function tests/test_host_cpu.py restates in uint64.  True = kept."""
    with np.errstate(over="ignore"):
        one = np.ones(1, np.uint32)
        r = _mix(np.uint32(seed) ^ (np.arange(rows, dtype=np.uint32) * np.uint32(0x9e3779b1)))[:, None]
        j = np.arange(cols, dtype=np.uint32)
        kk = j & np.uint32(31)
        c = _mix((j >> np.uint32(5)) * np.uint32(0x85ebca77) + np.uint32(0x6a09e667))
        c = c ^ _mix(np.uint32(0x3c6ef372) + ((kk & np.uint32(3)) | ((kk >> np.uint32(3)) << np.uint32(2))))
        c = (c ^ np.where((kk & np.uint32(4)) != 0, _mix(np.uint32(0xa54ff53a) * one), np.uint32(0)))[None, :]
        h = ((r ^ c) & np.uint32(0xffffff)) * np.uint32(0x9E3779)
        h = h ^ (h >> np.uint32(16))
        h = (h & np.uint32(0xffffff)) * np.uint32(0x85EBCB)
    t = math.ceil(float(np.float32(p)) * 2.0 ** 24)
    thr = 0xffffffff if t >= 2 ** 24 else t << 8
    return h >= np.uint32(thr)


def case_masks(case, p):
    """keep [T][B][H][Lq][Lk] (bool) with the hook's row numbering: row = (b * H + h) * Lq + i in the stream seeds[t]."""
    c = CASES[case]
    B, H, Lq, Lk = c["B"], c["H"], c["Lq"], c["Lk"]
    return np.stack([keep_mask(s, B * H * Lq, Lk, p).reshape(B, H, Lq, Lk) for s in drop_seeds(case)])


# ------------------------------------------------------------------------------------------------ the values a cache holds
def cache_values(k, v, cache, kind):
    """K / V as the backward reads them out of the forward's cache (kv_layout.hpp), exactly, as float64 arrays:
    0 / 3: the fp32 values (the split cache's hi + lo pair carries them to 2^-20: part of the bound);
    1: rounded to nearest fp16 / bf16;  8: V = fp16(v) to nearest, K = hi16 + e4m3((k - hi16) 2^10) 2^-10 with hi16 = fp16(k) rounded
    toward zero (the helpers of tests/emulate_attention_arithmetic.py)."""
    kt, vt = torch.from_numpy(k), torch.from_numpy(v)
    if cache in (0, 3):
        return k.astype(np.float64), v.astype(np.float64)
    if cache == 1:
        dt = torch.bfloat16 if kind == BF16 else torch.float16
        return kt.to(dt).double().numpy(), vt.to(dt).double().numpy()
    assert cache == 8
    import emulate_attention_arithmetic as E
    hi = E._rtz16(kt)
    return (hi + E._e4(kt.double() - hi, 1024.0)).numpy(), vt.half().double().numpy()


# ------------------------------------------------------------------------------------------------ the float64 oracle
def oracle(q, k, v, dO, keep=None, p=0.0, chunk=8):
    """q, dO [T][B][H][Lq][dh], k, v [B][H][Lk][dh] (any float type; computed in float64), keep [T][B][H][Lq][Lk] bool or None.
    Returns a dict of float64 arrays: O [T][B][H][Lq][dh], lse2, D, Theta [T][B][H][Lq], dQ, A_dQ like q, dK, dV, A_dK, A_dV like k,
    the floor sums sT_q [T][B][H][Lq] (sum_j T), sT_k, sPd_k [B][H][Lk] (sum over t, i of T / of Pd), and the scalars smax (max |s2|),
    sigma (max over (i, j) of log2(e) / sqrt(dh) * sum_d |q_d k_d|), lmax (max |lse2|), dsmax (max |dS|)."""
    tq, tk, tv, tdo = (torch.as_tensor(np.asarray(x, np.float64)) for x in (q, k, v, dO))
    T, B, H, Lq, dh = tq.shape
    cn = 1.0 / math.sqrt(dh)
    ks = 1.0 / (1.0 - p) if keep is not None else 1.0
    o = dict(O=torch.zeros_like(tq), lse2=torch.zeros(T, B, H, Lq, dtype=torch.float64), dQ=torch.zeros_like(tq), A_dQ=torch.zeros_like(tq),
             dK=torch.zeros_like(tk), dV=torch.zeros_like(tk), A_dK=torch.zeros_like(tk), A_dV=torch.zeros_like(tk))
    for n in ("D", "Theta", "sT_q"):
        o[n] = torch.zeros(T, B, H, Lq, dtype=torch.float64)
    for n in ("sT_k", "sPd_k"):
        o[n] = torch.zeros(tk.shape[:3], dtype=torch.float64)
    smax = sigma = lmax = dsmax = 0.0
    for b0 in range(0, B, chunk):
        sl = slice(b0, min(B, b0 + chunk))
        kb, vb = tk[sl], tv[sl]
        kT, vT, ka = kb.transpose(-1, -2), vb.transpose(-1, -2), kb.abs()
        for t in range(T):
            qb, ob = tq[t, sl], tdo[t, sl]
            S = (qb @ kT) * cn
            m = S.max(-1, keepdim=True).values
            E = torch.exp(S - m)
            Z = E.sum(-1, keepdim=True)
            P = E / Z
            lse2 = ((m + torch.log(Z)) * LOG2E).squeeze(-1)
            smax = max(smax, float(S.abs().max()) * LOG2E)
            sigma = max(sigma, float((qb.abs() @ ka.transpose(-1, -2)).max()) * cn * LOG2E)
            del S, E
            km = torch.from_numpy(keep[t, sl]).to(torch.float64) * ks if keep is not None else None
            Pd = P * km if km is not None else P
            O = Pd @ vb
            D = (ob * O).sum(-1)
            Theta = (ob * O).abs().sum(-1)
            dP = ob @ vT
            Psi = ob.abs() @ vb.abs().transpose(-1, -2)
            if km is not None:
                dP *= km
                Psi *= km
            dS = P * (dP - D.unsqueeze(-1))
            Tm = P * (Psi + Theta.unsqueeze(-1))
            del dP, Psi
            dsmax = max(dsmax, float(dS.abs().max()))
            o["O"][t, sl], o["lse2"][t, sl], o["D"][t, sl], o["Theta"][t, sl] = O, lse2, D, Theta
            o["dQ"][t, sl] = (dS @ kb) * cn
            o["A_dQ"][t, sl] = (Tm @ ka) * cn
            o["sT_q"][t, sl] = Tm.sum(-1)
            o["dK"][sl] += (dS.transpose(-1, -2) @ qb) * cn
            o["A_dK"][sl] += (Tm.transpose(-1, -2) @ qb.abs()) * cn
            o["dV"][sl] += Pd.transpose(-1, -2) @ ob
            o["A_dV"][sl] += Pd.transpose(-1, -2) @ ob.abs()
            o["sT_k"][sl] += Tm.sum(-2)
            o["sPd_k"][sl] += Pd.sum(-2)
            lmax = max(lmax, float(lse2.abs().max()))
    out = {n: x.numpy() for n, x in o.items()}
    out.update(smax=smax, sigma=sigma, lmax=lmax, dsmax=dsmax)
    return out


def oscale(dO):
    """The power-of-two gradient scale of the split-precision kernels (oscale_kernel): 2^(10 - exponent(max |dO|)); 1 for dO = 0."""
    mx = float(np.abs(dO).max())
    return 2.0 ** (10 - math.frexp(mx)[1]) if 0.0 < mx < 3.0e38 else 1.0


# ------------------------------------------------------------------------------------------------ the bounds
def bounds(family, inp, orc, dh, n_it, Lq, Lk):
    """Per-element bounds |error| <= alpha * A + beta of dQ, dK and dV for one kernel family, from its arithmetic (u = 2^-24).

    The probability.  P = exp2(s2 - lse2) with s2 = log2(e) / sqrt(dh) * q.k.  Absolute error of the exponent:
      fp32 families: the dh-term dot product, its scaling and the subtraction, (dh + 2) u sigma + 2 u (smax + lmax), plus the fp32
        rounding of the lse handed in, u lmax;
      split-precision families: q and k enter as fp16 hi + lo pairs with BOTH halves rounded toward zero (2^-20 each), the lo.lo
        product is dropped (2^-20), then an fp32 accumulation: sigma (3 * 2^-20 + (dh + 3) u); a lo half below the fp16 normals loses
        up to 2^-24 absolute per element: log2(e) / sqrt(dh) * 2^-24 (max |q|_1 + max |k|_1); the same lse terms.
    eps_P = ln 2 * that + 2^-22 (the hardware exp2 is good to an ulp of fp32; 2^-22 leaves two).
    The gradients.  dP and D are dh-term fp32 dot products, the outer contraction has Kc terms (Kc = Lk for dQ, n_it * Lq for dK and dV;
    atomics and partial sums reorder them, the bound does not depend on the order): (dh + Kc + 8) u relative to A.
      fp32 families (head dim 32, MFMA fp32, materialised): alpha = eps_P + (dh + Kc + 8) u, beta = 0.
      three-term split families (attn_bwd_split_kernel, attn_bwd_batched_256): every product has two operand pairs at 2^-20 and a
        dropped lo.lo at 2^-20, dP and the gradient product in sequence: + 2^-17.
      attn_bwd_split2_kernel (kGrad1): P' = 2^14 P and dS' = oscale dS enter the three gradient products as ONE fp16 value rounded to
        nearest: + 2^-11 per term, the dominant term.
    beta (split-precision families only): 16-bit values below the fp16 normals (2^-14) carry an absolute error up to 2^-24:
        dS' -> 2^-24 / oscale per term of dQ and dK;  P' -> 2^-38 per term of dV;  the lo halves of q, k and oscale dO -> 2^-24
        (2^-24 / oscale) per term against sum T (sum Pd).  attn_bwd_batched_256 rescales dS' by a second power of two taken from
        max |dS'| before its dQ product: the floor is then up to 2^-33 max |dS|; the larger of the two is used.
    A single-product or stage cache adds nothing: the oracle differentiates through the values the cache holds."""
    q, k, dO = (np.abs(inp[n]).astype(np.float64) for n in ("q", "k", "dO"))
    cn, c2 = 1.0 / math.sqrt(dh), LOG2E / math.sqrt(dh)
    sigma, smax, lmax = orc["sigma"], orc["smax"], orc["lmax"]
    lse_terms = 2 * U * (smax + lmax) + U * lmax
    split = family in (FAM_SPLIT, FAM_SPLIT2, FAM_B256)
    if split:
        eps_e = sigma * (3 * 2.0 ** -20 + (dh + 3) * U) + c2 * 2.0 ** -24 * (q.sum(-1).max() + k.sum(-1).max()) + lse_terms
    else:
        eps_e = (dh + 2) * U * sigma + lse_terms
    eps_p = math.log(2.0) * eps_e * 1.01 + 2.0 ** -22
    extra = {FAM_SPLIT: 2.0 ** -17, FAM_B256: 2.0 ** -17, FAM_SPLIT2: 2.0 ** -17 + 2.0 ** -11 * (1 + 2.0 ** -10)}.get(family, 0.0)
    T = max(1, n_it)
    alpha = {"dQ": eps_p + extra + (dh + Lk + 8) * U, "dK": eps_p + extra + (dh + T * Lq + 8) * U}
    alpha["dV"] = alpha["dK"]
    out = {n: alpha[n] * orc["A_" + n] for n in alpha}
    if split:
        fl = 2.0 ** -24 / oscale(inp["dO"])
        fq = max(fl, 2.0 ** -33 * orc["dsmax"]) if family == FAM_B256 else fl
        out["dQ"] = out["dQ"] + cn * (fq * k.sum(-2)[None, :, :, None, :] + 2.0 ** -24 * orc["sT_q"][..., None])
        out["dK"] = out["dK"] + cn * (fl * q.sum((0, 3))[:, :, None, :] + 2.0 ** -24 * orc["sT_k"][..., None])
        out["dV"] = out["dV"] + 2.0 ** -38 * dO.sum((0, 3))[:, :, None, :] + fl * orc["sPd_k"][..., None]
    out["alpha"] = alpha
    return out


def d_bound(orc, dh):
    """D = rowsum(dO * O) in fp32 from the fp32-rounded O: (dh + 4) u sum_d |dO_d O_d|."""
    return (dh + 4) * U * orc["Theta"]


# ------------------------------------------------------------------------------------------------ the C ABI
def plan_of(lib, case, spec=None):
    """The plan record of a case, from the hook with NULL data pointers (no device is touched)."""
    c = CASES[case]
    s = spec or _spec(case)
    plan = (C.c_int32 * 4)(-1, -1, -1, -1)
    nul = [None] * 6
    fake = C.c_void_p(1 << 20)                       # never read: the plan is returned ahead of every device call
    if c["launcher"] == "batched":
        seeds = (C.c_uint32 * 16)(*drop_seeds(case))
        rc = lib.parq_k_attention_backward_batched(*nul, c["B"], c["H"], c["Lq"], c["Lk"], c["dh"], c["n_it"], s["cache"], s["kind"],
                                                   s["drop"], seeds, None, None, None, 0, None, None, plan, None)
    else:
        det = det_scratch_bytes(c) if s["det"] else 0
        rc = lib.parq_k_attention_backward(*nul, c["B"], c["H"], c["Lq"], c["Lk"], c["dh"], s["layout"], s["acc"], c["use_absmax"],
                                           s["drop"], 0, None, None, None, None, 0, fake if det else None, det, None, None, plan, None)
    assert rc == 0, lib.parq_last_error()
    return tuple(plan)


def det_scratch_bytes(c):
    return c["B"] * c["H"] * -(-c["Lk"] // 64) * ((c["Lq"] + 31) // 32 * 32) * 64 * 4

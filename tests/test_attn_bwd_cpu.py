"""CPU tier of the attention backward tests (tests/attn_bwd_cases.py): the spelled-out float64 oracle against autograd and central
differences, A as a bound of |gradient|, the dropout mask's row numbering, and — without a device — the plan record of every case of
the table, the argument checks of the two entry points and their scratch size."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import attn_bwd_cases as A
from oracle import parq_oracle as O
from parq_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("parq_k_attention_backward_scratch_bytes", "parq_k_attention_backward", "parq_k_attention_backward_batched")


def _small(seed, T=2, B=2, H=2, Lq=5, Lk=7, dh=8):
    g = np.random.Generator(np.random.PCG64(seed))
    return dict(q=g.standard_normal((T, B, H, Lq, dh)), k=g.standard_normal((B, H, Lk, dh)), v=g.standard_normal((B, H, Lk, dh)),
                dO=g.standard_normal((T, B, H, Lq, dh)))


def _tokens(x):            # [B][H][L][dh] -> [B][L][H*dh]
    B, H, L, dh = x.shape
    return x.permute(0, 2, 1, 3).reshape(B, L, H * dh)


def _autograd(inp, keep, p):
    """The same gradients from float64 autograd: oracle.parq_oracle.mha with identity projections where there is no mask, the lines
    of its body with the mask on the probabilities where there is one."""
    q, k, v, dO = (torch.tensor(inp[n], dtype=torch.float64) for n in ("q", "k", "v", "dO"))
    T, B, H, Lq, dh = q.shape
    Cn = H * dh
    k.requires_grad_(True), v.requires_grad_(True), q.requires_grad_(True)
    eye3, zero3, eye = torch.eye(Cn, dtype=torch.float64).repeat(3, 1), torch.zeros(3 * Cn, dtype=torch.float64), torch.eye(Cn, dtype=torch.float64)
    loss, outs = 0.0, []
    for t in range(T):
        if keep is None:
            o = O.mha(_tokens(q[t]), _tokens(k), _tokens(v), eye3, zero3, eye, torch.zeros(Cn, dtype=torch.float64), H)
            o = o.view(B, Lq, H, dh).transpose(1, 2)
        else:
            a = torch.softmax((q[t] * (1.0 / math.sqrt(dh))) @ k.transpose(-1, -2), dim=-1)
            o = (a * torch.from_numpy(keep[t]).double() / (1.0 - p)) @ v
        outs.append(o.detach())
        loss = loss + (o * dO[t]).sum()
    loss.backward()
    return q.grad.numpy(), k.grad.numpy(), v.grad.numpy(), torch.stack(outs).numpy()


@pytest.mark.parametrize("p", [0.0, 0.25])
def test_spelled_out_oracle_equals_float64_autograd(p):
    inp = _small(3)
    keep = None if p == 0 else np.stack([A.keep_mask(11 + t, 2 * 2 * 5, 7, p).reshape(2, 2, 5, 7) for t in range(2)])
    assert keep is None or (0.5 < keep.mean() < 0.95)
    o = A.oracle(inp["q"], inp["k"], inp["v"], inp["dO"], keep, p, chunk=1)
    gq, gk, gv, out = _autograd(inp, keep, p)
    for got, want in ((o["dQ"], gq), (o["dK"], gk), (o["dV"], gv), (o["O"], out)):
        assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
    S = np.einsum("tbhid,bhjd->tbhij", inp["q"], inp["k"]) / math.sqrt(8)
    assert np.abs(o["lse2"] - np.log2(np.exp(S).sum(-1))).max() < 1e-12
    assert np.abs(o["D"] - (inp["dO"] * o["O"]).sum(-1)).max() < 1e-13


def test_oracle_agrees_with_central_differences_on_a_tiny_case():
    inp = _small(5, T=1, B=1, H=1, Lq=3, Lk=4, dh=4)
    keep = np.array([[1, 1, 0, 1], [0, 1, 1, 1], [1, 1, 1, 0]], bool).reshape(1, 1, 1, 3, 4)
    o = A.oracle(inp["q"], inp["k"], inp["v"], inp["dO"], keep, 0.25)
    f = lambda x: float((A.oracle(x["q"], x["k"], x["v"], x["dO"], keep, 0.25)["O"] * inp["dO"]).sum())
    h = 1e-6
    for name, grad in (("q", o["dQ"]), ("k", o["dK"]), ("v", o["dV"])):
        for idx in np.ndindex(inp[name].shape):
            hi, lo = {n: x.copy() for n, x in inp.items()}, {n: x.copy() for n, x in inp.items()}
            hi[name][idx] += h
            lo[name][idx] -= h
            assert abs((f(hi) - f(lo)) / (2 * h) - grad[idx]) < 1e-8, (name, idx)


def test_A_bounds_the_gradient_elementwise_and_the_floor_sums_are_what_they_say():
    for p in (0.0, 0.25):
        inp = _small(9, T=3, Lq=6, Lk=40, dh=16)
        inp["k"][:, :, 39] = 3.0 * inp["q"][0, :, :, 5]                      # a peaky row
        keep = None if p == 0 else np.stack([A.keep_mask(5 + t, 2 * 2 * 6, 40, p).reshape(2, 2, 6, 40) for t in range(3)])
        o = A.oracle(inp["q"], inp["k"], inp["v"], inp["dO"], keep, p)
        for n in ("dQ", "dK", "dV"):
            assert (np.abs(o[n]) <= o["A_" + n] * (1 + 1e-12)).all() and (o["A_" + n] > 0).all()
        assert (np.abs(o["D"]) <= o["Theta"] * (1 + 1e-12)).all()
        S2 = np.einsum("tbhid,bhjd->tbhij", inp["q"], inp["k"]) / 4.0 * A.LOG2E
        assert abs(o["smax"] - np.abs(S2).max()) < 1e-9 and o["sigma"] >= o["smax"] and abs(o["lmax"] - np.abs(o["lse2"]).max()) < 1e-12
        assert np.allclose(o["sPd_k"].sum(-1), 3 * 6, rtol=0.5 if p else 1e-12)      # rows of P sum to 1 (kept share ~ 1 with dropout)


def test_oscale_is_the_kernels_power_of_two():
    """oscale_kernel: frexp(max) = (m, ex), m in [0.5, 1): scale = 2^(10 - ex) puts max |dO| into [2^9, 2^10); 1 for a zero gradient."""
    for mx in (1.0, 0.75, 3.9, 2.0 ** -20 * 3.3, 2.0 ** 20 * 5.1, 1e-30):
        s = A.oscale(np.array([mx, -mx / 3], np.float32))
        assert math.log2(s) == int(math.log2(s)) and 2.0 ** 9 <= np.float32(mx) * s < 2.0 ** 10
    assert A.oscale(np.zeros(4, np.float32)) == 1.0


def test_mask_restatement_matches_the_one_of_test_host_cpu_and_rows_are_numbered_by_scene_head_query():
    """keep_mask in uint32 equals the uint64 restatement written out in test_host_cpu.py (repeated here for p = 0.1, its seed and
    size), and case_masks numbers the rows bh * Lq + i: row (b, h, i) of iteration t is row (b * H + h) * Lq + i of stream seeds[t]."""
    M = np.uint64(0xFFFFFFFF)
    u32 = lambda x: (x & M).astype(np.uint64)

    def mix(x):
        x = u32(x); x ^= x >> np.uint64(16); x = u32(x * np.uint64(0x7feb352d)); x ^= x >> np.uint64(15)
        x = u32(x * np.uint64(0x846ca68b)); x ^= x >> np.uint64(16)
        return x
    p, rows, cols, seed = 0.1, 512, 4096, 12345
    thr = np.uint64(int(np.ceil(p * 2 ** 24)) << 8)
    with np.errstate(over="ignore"):
        r = mix(np.uint64(seed) ^ u32(np.arange(rows, dtype=np.uint64) * np.uint64(0x9e3779b1)))[:, None]
        j = np.arange(cols, dtype=np.uint64)
        k = j & np.uint64(31)
        c = mix(u32((j >> np.uint64(5)) * np.uint64(0x85ebca77) + np.uint64(0x6a09e667)))
        c = c ^ mix(np.uint64(0x3c6ef372) + ((k & np.uint64(3)) | ((k >> np.uint64(3)) << np.uint64(2))))
        c = (c ^ np.where((k & np.uint64(4)) != 0, mix(np.uint64(0xa54ff53a) + np.zeros(1, np.uint64)), np.uint64(0)))[None, :]
        h = u32(((r ^ c) & np.uint64(0xffffff)) * np.uint64(0x9E3779)); h ^= h >> np.uint64(16)
        h = u32((h & np.uint64(0xffffff)) * np.uint64(0x85EBCB))
    assert np.array_equal(A.keep_mask(seed, rows, cols, p), ~(h < thr))
    case = "g1_iters16"
    c = A.CASES[case]
    m = A.case_masks(case, 0.25)
    assert m.shape == (16, 1, 2, 24, 2049) and abs(m.mean() - 0.75) < 0.005
    seeds = A.drop_seeds(case)
    assert len(set(seeds)) == 16
    for t, b, hh, i in ((0, 0, 0, 0), (3, 0, 1, 7), (15, 0, 1, 23)):
        row = (b * c["H"] + hh) * c["Lq"] + i
        assert np.array_equal(m[t, b, hh, i], A.keep_mask(seeds[t], row + 1, c["Lk"], 0.25)[row])
    assert not np.array_equal(m[0], m[1])


def test_cache_values_are_the_16_bit_forms():
    g = np.random.Generator(np.random.PCG64(2))
    k, v = g.standard_normal((1, 1, 64, 64), dtype=np.float32), g.standard_normal((1, 1, 64, 64), dtype=np.float32)
    for cache in (0, 3):
        kk, vv = A.cache_values(k, v, cache, A.F16)
        assert np.array_equal(kk, k.astype(np.float64)) and np.array_equal(vv, v.astype(np.float64))
    kk, vv = A.cache_values(k, v, 1, A.F16)
    assert np.array_equal(kk, k.astype(np.float16).astype(np.float64)) and np.abs(kk - k).max() <= 2.0 ** -11 * np.abs(k).max()
    kk, _ = A.cache_values(k, v, 1, A.BF16)
    assert (np.abs(kk - k) <= 2.0 ** -8 * np.abs(k)).all() and not np.array_equal(kk, k)
    k8, v8 = A.cache_values(k, v, 8, A.F16)
    assert np.array_equal(v8, v.astype(np.float16).astype(np.float64))
    # hi16 rounds toward zero (residual < 2^-10 |k|), the e4m3 residual keeps 4 significant bits of it, or 2^-20 absolute
    assert (np.abs(k8 - k) <= 2.0 ** -14 * np.abs(k) + 2.0 ** -20).all() and np.abs(k8 - k).max() > 2.0 ** -20


# ------------------------------------------------------------------------------------------------ the entry points, no device
def test_every_case_of_the_table_reaches_the_path_it_is_named_for():
    """The plan record — from attn_bwd_kb_group, attn_bwd_dq_partial_floats and the head-dim-256 scratch size, returned for NULL data
    pointers — names the family, key blocks per workgroup, slot count and QP that the case table claims."""
    lib = _lib.load()
    seen = set()
    for name, c in A.CASES.items():
        assert A.plan_of(lib, name) == c["plan"], name
        seen.add(c["plan"][:2])
    assert {(A.FAM_SPLIT2, 4), (A.FAM_SPLIT2, 2), (A.FAM_SPLIT2, 1), (A.FAM_B256, 1), (A.FAM_VALU32, 1), (A.FAM_MFMA2, 1), (A.FAM_MFMA8, 1),
            (A.FAM_SPLIT, 1), (A.FAM_MAT, 1)} == seen
    # the shapes behind the claims: partial last groups, the second 512-row slice, kMaxBwdIters, ragged and whole last blocks
    nkb = lambda n: -(-A.CASES[n]["Lk"] // 256)
    assert nkb("g4_whole") == 16 and A.CASES["g4_whole"]["Lk"] % 256 == 0
    assert nkb("g4_ragged") == 18 and nkb("g4_ragged") % 4 == 2 and A.CASES["g4_ragged"]["Lk"] % 256 == 148
    assert nkb("g2_stage") == 10 and A.CASES["g2_stage"]["Lk"] % 64 == 0 and A.CASES["g2_stage"]["Lk"] % 256 != 0
    assert nkb("g2_whole") == 9 and A.CASES["g2_whole"]["Lk"] % 256 == 0 and A.CASES["g2_whole"]["n_it"] == 1
    assert A.CASES["g1_iters16"]["n_it"] == 16 and A.CASES["g1_iters16"]["Lk"] % 256 == 1
    c = A.CASES["b256_two_slices"]
    assert 512 < c["n_it"] * c["Lq"] < 1024
    # the deterministic form of the short-key kernel: one slot per 64 keys
    for s in A.specs():
        if s["det"]:
            assert A.plan_of(lib, s["case"], s) == (A.FAM_MFMA2, 1, -(-A.CASES[s["case"]]["Lk"] // 64), 0)
    specs = A.specs()
    assert {s["cache"] for s in specs} == {0, 1, 3, 8} and any(s["kind"] == A.BF16 for s in specs)
    for s in specs:
        c = A.CASES[s["case"]]
        if s["cache"]:
            assert c["launcher"] == "batched" and c["dh"] == 64 and (s["cache"] != 8 or c["Lk"] % 64 == 0)


def test_kb_group_switches_where_the_formula_says():
    lib = _lib.load()
    plan = (C.c_int32 * 4)()
    for B, H, Lk in ((32, 4, 4096), (32, 4, 4097), (32, 4, 2304), (32, 4, 2048), (8, 4, 4096), (16, 4, 8192), (64, 8, 2048), (1, 2, 2049)):
        nkb, g = -(-Lk // 256), 4
        while g > 1 and B * H * -(-nkb // g) < 512:
            g >>= 1
        assert lib.parq_k_attention_backward_batched(None, None, None, None, None, None, B, H, 40, Lk, 64, 2, 0, 0, 0.0, None, None, None,
                                                     None, 0, None, None, plan, None) == 0
        assert tuple(plan) == (A.FAM_SPLIT2, g, -(-nkb // g), 0), (B, H, Lk)


def test_header_binding_and_library_agree_on_the_entry_points():
    hdr = open(os.path.join(ROOT, "include", "parq_hip.h")).read()
    api = open(os.path.join(ROOT, "parq_amd", "csrc", "api.hip")).read()
    lib = _lib.load()
    for name in NEW:
        m = re.search(r"\b(?:int|size_t)\s+\(%s\)\s*\(([^;]*)\)\s*;" % name, hdr)
        assert m, "include/parq_hip.h must declare %s with a parenthesised name" % name
        params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
        res, args = _lib.EXTRA_SYMBOLS[name]
        assert name not in _lib.SYMBOLS and len(args) == len(params) and res is (C.c_size_t if name.endswith("bytes") else C.c_int)
        for p, a in zip(params, args):
            if "*" in p:
                assert a in (C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_uint32)), (name, p)
            else:
                assert a is {"int32_t": C.c_int32, "uint32_t": C.c_uint32, "float": C.c_float, "size_t": C.c_size_t,
                             "parq_stream": C.c_void_p}[p.split()[0]], (name, p)
        d = re.search(r"\b(?:int|size_t)\s+%s\s*\(([^)]*)\)\s*\{" % name, api)
        assert d, "parq_amd/csrc/api.hip must define %s" % name
        types = lambda s: [re.sub(r"\s+", " ", re.sub(r"\w+$", "", p.strip()).replace(" *", "*")).strip() for p in s.replace("\n", " ").split(",")]
        assert types(d.group(1)) == types(m.group(1)), name
        fn = getattr(lib, name)
        assert fn.argtypes == args and fn.restype is res


def _single(lib, **kw):
    p = C.c_void_p(1 << 20)                                  # never read: every refusal returns ahead of the first device call
    a = dict(q=p, k=p, v=p, dO=p, O=p, lse=p, B=2, H=2, Lq=5, Lk=70, dh=64, layout=1, acc=0, absmax=0, drop=0.0, seed=1, gq=p, gk=p, gv=p,
             scratch=p, nbytes=1 << 40, det=None, det_bytes=0, D=None, masks=None, plan=None)
    a.update(kw)
    return lib.parq_k_attention_backward(a["q"], a["k"], a["v"], a["dO"], a["O"], a["lse"], a["B"], a["H"], a["Lq"], a["Lk"], a["dh"], a["layout"],
                                         a["acc"], a["absmax"], a["drop"], a["seed"], a["gq"], a["gk"], a["gv"], a["scratch"], a["nbytes"],
                                         a["det"], a["det_bytes"], a["D"], a["masks"], a["plan"], None)


def _batched(lib, **kw):
    p = C.c_void_p(1 << 20)
    a = dict(q=p, k=p, v=p, dO=p, O=p, lse=p, B=1, H=2, Lq=5, Lk=2112, dh=64, n_it=2, cache=0, kind=0, drop=0.0, seeds=(C.c_uint32 * 16)(),
             gq=p, gkv=p, scratch=p, nbytes=1 << 40, D=None, masks=None, plan=None)
    a.update(kw)
    return lib.parq_k_attention_backward_batched(a["q"], a["k"], a["v"], a["dO"], a["O"], a["lse"], a["B"], a["H"], a["Lq"], a["Lk"], a["dh"],
                                                 a["n_it"], a["cache"], a["kind"], a["drop"], a["seeds"], a["gq"], a["gkv"], a["scratch"],
                                                 a["nbytes"], a["D"], a["masks"], a["plan"], None)


def test_entry_points_refuse_bad_arguments_before_any_launch():
    lib = _lib.load()
    p = C.c_void_p(1 << 20)
    need = A.det_scratch_bytes(dict(B=2, H=2, Lq=5, Lk=70))
    ARG, WS = 1, 4
    for kw in (dict(B=0), dict(H=0), dict(Lq=0), dict(Lk=0), dict(dh=48), dict(dh=512), dict(layout=2), dict(layout=-1), dict(acc=2),
               dict(absmax=-1), dict(drop=1.0), dict(drop=-0.1), dict(drop=float("nan")), dict(det=p, det_bytes=0), dict(det=None, det_bytes=need),
               dict(det=p, det_bytes=need - 4), dict(det=C.c_void_p((1 << 20) + 4), det_bytes=need), dict(det=p, det_bytes=need, dh=32),
               dict(det=p, det_bytes=1 << 30, dh=128), dict(q=None), dict(lse=None), dict(gv=None), dict(scratch=None), dict(masks=p)):
        assert _single(lib, **kw) == ARG and lib.parq_last_error(), kw
    sz = lib.parq_k_attention_backward_scratch_bytes(2, 2, 5, 70, 64, 0, 0)
    assert sz > 0 and _single(lib, nbytes=sz - 1) == WS and _single(lib, nbytes=sz, scratch=C.c_void_p((1 << 20) + 8)) == WS
    for kw in (dict(B=0), dict(n_it=0), dict(n_it=17), dict(dh=32), dict(dh=128), dict(Lk=2047), dict(cache=2), dict(cache=8, Lk=2100),
               dict(cache=3, dh=256), dict(kind=2), dict(kind=1, cache=3), dict(kind=1, cache=0), dict(drop=1.0), dict(drop=0.25, seeds=None),
               dict(v=None), dict(gkv=None), dict(scratch=None), dict(masks=p)):
        assert _batched(lib, **kw) == ARG and lib.parq_last_error(), kw
    sz = lib.parq_k_attention_backward_scratch_bytes(1, 2, 5, 2112, 64, 2, 0)
    assert sz > 0 and _batched(lib, nbytes=sz - 1) == WS
    # the plan alone is served with NULL data pointers; without a plan NULL data is refused
    plan = (C.c_int32 * 4)()
    assert _batched(lib, q=None, plan=plan) == 0 and _batched(lib, q=None) == ARG
    assert _single(lib, q=None, plan=plan) == 0 and tuple(plan) == (A.FAM_MFMA2, 1, 0, 0)


def test_scratch_size_covers_each_component_and_is_monotone():
    lib = _lib.load()
    size = lib.parq_k_attention_backward_scratch_bytes
    pad = lambda n: (n + 31) // 32 * 32
    for c in A.CASES.values():
        B, H, Lq, Lk, dh, T = c["B"], c["H"], c["Lq"], c["Lk"], c["dh"], c["n_it"]
        fam, g, slots, QP = c["plan"]
        base = size(B, H, Lq, Lk, dh, T, 0)
        comp = [max(1, T) * B * H * pad(Lq), 2, max(1, T) * B * H * slots * pad(Lq) * 64]                    # D, the scale words, dQ partials
        if fam == A.FAM_SPLIT2:
            comp.append(T * B * H * (pad(Lq) // 32) * 8448 // 2)                                              # pack images
        if fam == A.FAM_B256:
            comp.append(2 * Lk * QP + 1024 + QP * 1024 + QP * 256 + QP + 16)                                  # attn_bwd_batched256_scratch_floats
        if fam == A.FAM_MAT:
            comp.append(2 * Lq * ((Lk + 15) // 16 * 16) + dh * ((Lk + 15) // 16 * 16))                        # attn_bwd_mat_scratch_floats
        assert base >= 4 * sum(comp), c["name"]
        assert base <= 4 * (sum(comp) + 64 * 8), c["name"]                                                    # ... and nothing unexplained
        assert base % 256 == 0
        assert size(B, H, Lq + 32, Lk, dh, T, 0) >= base and size(B + 1, H, Lq, Lk, dh, T, 0) >= base      # (parts round up to 64 floats)
        assert size(B, H, Lq + 512, Lk, dh, T, 0) > base and size(B + 64, H, Lq, Lk, dh, T, 0) > base
        assert size(B, H, Lq, Lk + 256, dh, T, 0) >= base
        if fam == A.FAM_SPLIT2:
            blocks = -(-Lk // 32)
            assert size(B, H, Lq, Lk, dh, T, 3) - base == B * H * blocks * 16384 + 256                        # split cache + its flag
            assert size(B, H, Lq, Lk, dh, T, 1) - base == B * H * blocks * 8192 + 256
            assert size(B, H, Lq, Lk, dh, T, 8) == size(B, H, Lq, Lk, dh, T, 3)
            assert size(B, H, Lq, Lk, dh, T + 1 if T < 16 else T, 0) >= base
    assert size(0, 2, 5, 70, 64, 0, 0) == 0 and size(2, 2, 5, 70, 48, 0, 0) == 0 and size(2, 2, 5, 70, 64, 17, 0) == 0
    assert size(2, 2, 5, 70, 64, 0, 3) == 0 and size(2, 2, 5, 70, 256, 2, 3) == 0 and size(2, 2, 5, 70, 64, 2, 2) == 0

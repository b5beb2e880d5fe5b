"""The attention backward kernels (parq_amd/csrc/attn_bwd.hip), one launcher call at a time through parq_k_attention_backward and
parq_k_attention_backward_batched, judged per element against the float64 oracle of tests/attn_bwd_cases.py on the cases of its table:
key-block groups of 4 and 2 with full and partial last groups, ragged and whole last blocks, 16 iterations, one query, the second
512-row slice of the head-dim-256 composition, the block edges of the single-call kernels in both layouts, every cache kind.

Per case (one launch, everything checked on it):
  * dQ, dK, dV: |error| <= alpha * A + beta for every element, alpha and beta derived from the family's arithmetic
    (attn_bwd_cases.bounds, whose docstring is the derivation); with accumulate_kv = 1 the expected value is pre-fill + gradient and
    the rounding of that sum, 2 u (|pre-fill| + |gradient|), is added.
  * the Frobenius-relative error of each tensor is at most FROB of its family: 4 x the largest value measured against the oracle on
    the first run (profiles/attn_bwd_errors.txt; inputs are seeded, only the order of atomics varies between runs), and at most the
    RMS form of the per-element bound.
  * D = rowsum(dO * O) agrees to (dh + 4) u sum |dO O|.
  * gK / gV (accumulate_kv = 0) and the whole scratch — dQ partial slots, pack images, head-dim-256 scratch — are pre-filled with NaN:
    no NaN may reach an output.  The padding of lse and the unused column blocks of the packed inputs are NaN as well.
  * every buffer lies between guard bands that must be intact; the column blocks of the packed self-attention buffers that the call
    does not own keep their pre-fill bit for bit.
  * with dropout the keep-masks the entry returns (launch_dropout_apply, row bh * Lq + i, stream seeds[t]) equal the NumPy
    restatement, and the oracle is evaluated with exactly those masks.
  * dO = 0: every gradient is exactly 0.0.
Each test prints a line `attn_bwd ...` with its figures before it asserts (pytest -s)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import attn_bwd_cases as A
from gpu_util import lib, sptr
from parq_amd import _lib

pytestmark = pytest.mark.gpu
GUARD_WORDS, GUARD = 256, 0x5A5AA5A5
SPECS = sorted(A.specs(), key=lambda s: list(A.CASES).index(s["case"]))          # variants of a case next to each other: inputs built once

# Frobenius-relative error bounds per family (dQ, dK, dV): 4 x the measured maxima of profiles/attn_bwd_errors.txt
FROB = {"valu32": (9.7e-06, 3.8e-06, 5.5e-06), "mfma2": (8.2e-06, 6.7e-06, 6.6e-06), "mfma8": (6.4e-06, 5.6e-06, 7.6e-06),
        "split": (2.1e-05, 1.6e-05, 1.8e-05), "materialised": (2.7e-06, 3.2e-06, 2.6e-06), "split2": (3.7e-03, 1.2e-03, 1.1e-03),
        "batched256": (5.4e-06, 5.6e-06, 1.1e-05)}


@functools.lru_cache(maxsize=2)
def _inputs(case):
    return A.make_inputs(case)


@pytest.fixture(scope="module", autouse=True)
def _leave_nothing_behind():
    """The 32 x 4-scene cases hold a few GB of host and device buffers: give them back when the module is done."""
    yield
    _inputs.cache_clear()
    torch.cuda.empty_cache()


def _guarded(n, fill):
    """n floats filled with `fill` (a float, or a same-sized fp32 array) between two guard bands; returns (whole buffer, payload view)."""
    buf = torch.empty(n + 2 * GUARD_WORDS, dtype=torch.float32, device="cuda")
    w = buf.view(torch.int32)
    w[:GUARD_WORDS] = GUARD
    w[GUARD_WORDS + n:] = GUARD
    pay = buf[GUARD_WORDS:GUARD_WORDS + n]
    if isinstance(fill, float):
        pay.fill_(fill)
    else:
        pay.copy_(torch.from_numpy(np.ascontiguousarray(fill, np.float32).reshape(-1)))
    return buf, pay


def _guards_ok(buf):
    w = buf.view(torch.int32)
    return bool((w[:GUARD_WORDS] == GUARD).all().item() and (w[-GUARD_WORDS:] == GUARD).all().item())


def _p(t, off=0):
    return C.c_void_p(t.data_ptr() + 4 * off)


def _tok(x):            # [B][H][L][dh] -> [B][L][H * dh]
    B, H, L, dh = x.shape
    return np.ascontiguousarray(x.transpose(0, 2, 1, 3)).reshape(B, L, H * dh)


def _heads(t, H):       # torch [..., L, H * dh] -> numpy [..., H, L, dh]
    *lead, L, Cn = t.shape
    return t.reshape(*lead, L, H, Cn // H).transpose(-3, -2).contiguous().cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _variant_inputs(spec):
    inp = dict(_inputs(spec["case"]))
    if spec["do_zero"]:
        inp["dO"] = np.zeros_like(inp["dO"])
    elif spec["do_exp"]:
        inp["dO"] = inp["dO"] * np.float32(2.0 ** spec["do_exp"])                 # exact: a power of two
    return inp


def _reference(spec, inp):
    keep = A.case_masks(spec["case"], spec["drop"]) if spec["drop"] else None
    kc, vc = A.cache_values(inp["k"], inp["v"], spec["cache"], spec["kind"])
    return A.oracle(inp["q"], kc, vc, inp["dO"], keep, spec["drop"]), keep


def _launch(spec, inp, orc):
    """One call of the entry.  Returns gq [T][B][H][Lq][dh], gk, gv [B][H][Lk][dh], their pre-fills (None where NaN / zero), D, the masks
    (a CUDA bool tensor [T][B*H*Lq][Lk] and whether every value is 0 or 1 / (1 - p)), guard and untouched flags, the plan."""
    c = A.CASES[spec["case"]]
    B, H, Lq, Lk, dh, T = c["B"], c["H"], c["Lq"], c["Lk"], c["dh"], max(1, c["n_it"])
    Cn, lp = H * dh, (Lq + 31) // 32 * 32
    batched = c["launcher"] == "batched"
    nan = float("nan")
    O32, lse32 = orc["O"].astype(np.float32), orc["lse2"].astype(np.float32)
    lse_pad = np.full((T, B * H, lp), np.nan, np.float32)
    lse_pad[:, :, :Lq] = lse32.reshape(T, B * H, Lq)
    bufs = {}
    tok5 = lambda x: np.stack([_tok(x[t]) for t in range(T)])                      # [T][B][Lq][C]
    bufs["dO"], dO = _guarded(T * B * Lq * Cn, tok5(inp["dO"]))
    bufs["O"], Ot = _guarded(T * B * Lq * Cn, tok5(O32))
    bufs["lse"], lse = _guarded(lse_pad.size, lse_pad)
    nbytes = lib().parq_k_attention_backward_scratch_bytes(B, H, Lq, Lk, dh, c["n_it"], spec["cache"])
    assert nbytes > 0 and nbytes % 4 == 0
    bufs["scratch"], scratch = _guarded(nbytes // 4, nan)
    bufs["D"], D = _guarded(T * B * H * lp, nan)
    masks = None
    if spec["drop"]:
        bufs["masks"], masks = _guarded(T * B * H * Lq * Lk, nan)
    plan = (C.c_int32 * 4)(-1, -1, -1, -1)
    seeds = A.drop_seeds(spec["case"])
    pre_k = pre_v = None
    untouched = True
    if batched:
        bufs["q"], q = _guarded(T * B * Lq * Cn, tok5(inp["q"]))
        bufs["k"], k = _guarded(inp["k"].size, inp["k"])
        bufs["v"], v = _guarded(inp["v"].size, inp["v"])
        bufs["gq"], gq = _guarded(T * B * Lq * Cn, 0.0)
        bufs["gkv"], gkv = _guarded(B * Lk * 2 * Cn, nan)
        _lib.check(lib().parq_k_attention_backward_batched(_p(q), _p(k), _p(v), _p(dO), _p(Ot), _p(lse), B, H, Lq, Lk, dh, T, spec["cache"],
                                                          spec["kind"], spec["drop"], (C.c_uint32 * 16)(*seeds), _p(gq), _p(gkv),
                                                          _p(scratch), nbytes, _p(D), _p(masks) if masks is not None else None, plan, sptr()),
                   "attention_backward_batched")
        torch.cuda.synchronize()
        got_q = _heads(gq.view(T, B, Lq, Cn), H)
        g2 = gkv.view(B, Lk, 2, Cn)
        got_k, got_v = _heads(g2[:, :, 0], H), _heads(g2[:, :, 1], H)
    else:
        acc = spec["acc"]
        if spec["layout"] == A.CROSS:
            bufs["q"], q = _guarded(B * Lq * Cn, _tok(inp["q"][0]))
            bufs["k"], k = _guarded(inp["k"].size, inp["k"])
            bufs["v"], v = _guarded(inp["v"].size, inp["v"])
            qp, kp, vp = _p(q), _p(k), _p(v)
            bufs["gq"], gq = _guarded(B * Lq * Cn, 0.0)
            pre = A.prefill((B, Lk, 2, Cn), 11) if acc else None
            bufs["gkv"], gkv = _guarded(B * Lk * 2 * Cn, pre if acc else nan)
            gqp, gkp, gvp = _p(gq), _p(gkv), _p(gkv, Cn)
            if acc:
                pre_k, pre_v = _heads(torch.from_numpy(pre[:, :, 0]), H), _heads(torch.from_numpy(pre[:, :, 1]), H)
        else:
            qpack = np.full((B, Lq, 3, Cn), np.nan, np.float32)
            qpack[:, :, 0] = _tok(inp["q"][0])
            kvpack = np.full((B, Lk, 3, Cn), np.nan, np.float32)
            kvpack[:, :, 1], kvpack[:, :, 2] = _tok(inp["k"]), _tok(inp["v"])
            bufs["q"], q = _guarded(qpack.size, qpack)
            bufs["kv"], kv = _guarded(kvpack.size, kvpack)
            qp, kp, vp = _p(q), _p(kv, Cn), _p(kv, 2 * Cn)
            gq_pre = A.prefill((B, Lq, 3, Cn), 12)                                   # blocks 1, 2: not this call's
            gq_pre[:, :, 0] = 0.0
            gkv_pre = A.prefill((B, Lk, 3, Cn), 13)                                  # block 0: not this call's
            if not acc:
                gkv_pre[:, :, 1:] = np.nan
            bufs["gq"], gq = _guarded(gq_pre.size, gq_pre)
            bufs["gkv"], gkv = _guarded(gkv_pre.size, gkv_pre)
            gqp, gkp, gvp = _p(gq), _p(gkv, Cn), _p(gkv, 2 * Cn)
            if acc:
                pre_k, pre_v = _heads(torch.from_numpy(gkv_pre[:, :, 1]), H), _heads(torch.from_numpy(gkv_pre[:, :, 2]), H)
        det_bytes = A.det_scratch_bytes(c) if spec["det"] else 0
        if det_bytes:
            bufs["det"], det = _guarded(det_bytes // 4, nan)
        _lib.check(lib().parq_k_attention_backward(qp, kp, vp, _p(dO), _p(Ot), _p(lse), B, H, Lq, Lk, dh, spec["layout"], acc, c["use_absmax"],
                                                  spec["drop"], seeds[0], gqp, gkp, gvp, _p(scratch), nbytes,
                                                  _p(det) if det_bytes else None, det_bytes, _p(D), _p(masks) if masks is not None else None,
                                                  plan, sptr()), "attention_backward")
        torch.cuda.synchronize()
        if spec["layout"] == A.CROSS:
            got_q = _heads(gq.view(1, B, Lq, Cn), H)
            g2 = gkv.view(B, Lk, 2, Cn)
            got_k, got_v = _heads(g2[:, :, 0], H), _heads(g2[:, :, 1], H)
        else:
            g3, k3 = gq.view(B, Lq, 3, Cn), gkv.view(B, Lk, 3, Cn)
            got_q = _heads(g3[:, :, 0], H)[None]
            got_k, got_v = _heads(k3[:, :, 1], H), _heads(k3[:, :, 2], H)
            untouched = (np.array_equal(_bits(g3[:, :, 1:].cpu().numpy()), _bits(gq_pre[:, :, 1:])) and
                         np.array_equal(_bits(k3[:, :, 0].cpu().numpy()), _bits(gkv_pre[:, :, 0])))
    mask_ok = None
    if masks is not None:
        m = masks.view(T, B * H * Lq, Lk)
        inv = np.float32(1.0) / np.float32(1.0 - np.float32(spec["drop"]))
        mask_ok = bool(((m == 0) | (m == float(inv))).all().item())
        masks = m > 0
    return dict(gq=got_q, gk=got_k, gv=got_v, pre_k=pre_k, pre_v=pre_v, D=D.view(T, B, H, lp)[..., :Lq].cpu().numpy(), masks=masks, mask_ok=mask_ok,
                guards={n: _guards_ok(b) for n, b in bufs.items()}, untouched=untouched, plan=tuple(plan))


def _expected_plan(spec):
    c = A.CASES[spec["case"]]
    return (A.FAM_MFMA2, 1, -(-c["Lk"] // 64), 0) if spec["det"] else c["plan"]


@pytest.mark.parametrize("spec", SPECS, ids=[s["id"] for s in SPECS])
def test_gradients_against_the_float64_oracle(spec):
    c = A.CASES[spec["case"]]
    fam = c["plan"][0]
    inp = _variant_inputs(spec)
    orc, keep = _reference(spec, inp)
    r = _launch(spec, inp, orc)
    assert r["plan"] == _expected_plan(spec)
    assert all(r["guards"].values()), r["guards"]
    assert r["untouched"]
    if keep is not None:
        assert r["mask_ok"] and torch.equal(r["masks"].cpu(), torch.from_numpy(keep.reshape(r["masks"].shape)))
    got = {"dQ": r["gq"], "dK": r["gk"], "dV": r["gv"]}
    for n, g in got.items():
        assert np.isfinite(g).all(), n                                              # no NaN of a pre-fill, a slot or the scratch survives
    d_ratio = float((np.abs(r["D"].astype(np.float64) - orc["D"]) / np.maximum(A.d_bound(orc, c["dh"]), 1e-300)).max()) if not spec["do_zero"] else 0.0
    if spec["do_zero"]:
        assert (r["D"] == 0).all() and (got["dQ"] == 0).all()
        for n, pre in (("dK", r["pre_k"]), ("dV", r["pre_v"])):
            assert np.array_equal(_bits(got[n]), _bits(pre if pre is not None else np.zeros_like(got[n]))), n
        print("attn_bwd %-44s %-12s dO = 0: every gradient exactly zero" % (spec["id"], A.FAM_NAME[fam]))
        return
    bnd = A.bounds(fam, inp, orc, c["dh"], c["n_it"], c["Lq"], c["Lk"])
    figs, ok = [], d_ratio <= 1.0
    for i, n in enumerate(("dQ", "dK", "dV")):
        pre = {"dK": r["pre_k"], "dV": r["pre_v"]}.get(n)
        want, b = orc[n], bnd[n]
        if pre is not None:
            b = b + 2 * A.U * (np.abs(pre) + np.abs(want))
            want = want + pre.astype(np.float64)
        err = np.abs(got[n].astype(np.float64) - want)
        ratio = float((err / np.maximum(b, 1e-300)).max())
        norm = float(np.sqrt((orc[n] ** 2).sum()))
        if norm <= 2.0 ** -40 * float(np.sqrt((orc["A_" + n] ** 2).sum())):         # a single key: P = 1, dS = dP - D = 0, dQ = dK = 0 (the
            figs.append("%s ratio %.4f (the gradient vanishes: no relative error)" % (n, ratio))   # oracle's own roundoff is left): only the
            ok = ok and ratio <= 1.0                                               # per-element bound speaks
            continue
        frob, rms = float(np.sqrt((err ** 2).sum())) / norm, float(np.sqrt((b ** 2).sum())) / norm
        limit = FROB[A.FAM_NAME[fam]][i]
        figs.append("%s ratio %.4f frob %.3e (rms bound %.3e, asserted %.1e)" % (n, ratio, frob, rms, limit))
        ok = ok and ratio <= 1.0 and frob <= rms and frob <= limit
    print("attn_bwd %-44s %-12s D ratio %.4f | %s" % (spec["id"], A.FAM_NAME[fam], d_ratio, " | ".join(figs)))
    assert ok


DET = [s for s in SPECS if s["det"] and s["acc"] == 0]


@pytest.mark.parametrize("spec", DET, ids=[s["id"] for s in DET])
def test_deterministic_form_repeats_bit_for_bit(spec):
    """Two calls with the deterministic scratch give the same bits in dQ, dK and dV (the agreement with the oracle, within the same
    bounds as the atomic form, is test_gradients_against_the_float64_oracle on the same specs)."""
    inp = _variant_inputs(spec)
    orc, _ = _reference(spec, inp)
    a, b = _launch(spec, inp, orc), _launch(spec, inp, orc)
    assert a["plan"] == b["plan"] == _expected_plan(spec) and a["plan"][2] > 0
    for n in ("gq", "gk", "gv"):
        assert np.isfinite(a[n]).all() and np.array_equal(_bits(a[n]), _bits(b[n])), n

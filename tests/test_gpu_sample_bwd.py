"""The project-and-sample backward kernels (backward.hip: sample_bwd_kernel, sample_det_records_kernel, sample_det_gather_kernel)
called on their own through parq_k_project_sample_backward and judged per element against the float64 oracle, on the hand-placed
cases of tests/sample_bwd_cases.py: image borders, the sampled-but-not-valid bands, the depth clamp, a camera larger than the
feature grid, no valid view, tile seams, a second compaction round, a second list chunk, 17 views, 1024 channels, 16-bit tokens.

Both forms of every case: float atomics (no scratch) and the deterministic gather (a scratch of exactly the stated size with a guard
behind it).  The outputs are pre-filled with a non-zero pattern: the entry ADDS.

The bounds are derived from the arithmetic (sample_bwd_cases.token_bound / ref_bound / forward_bound), not from results.  Each test
prints its worst |error| / bound as a line `sample_bwd ratio ...` (pytest -s); profiles/sample_bwd_errors.txt keeps those lines.
No query is left out of any comparison except the named `gref_excluded` set (lattice points and the exact -1 / w limits, where the
bilinear sample has a kink) for the coordinate gradient; its size is asserted."""
import ctypes as C

import numpy as np
import pytest
import torch

import sample_bwd_cases as S
from gpu_util import dev, lib, sptr
from parq_amd import _lib

pytestmark = pytest.mark.gpu
FORMS = ("atomics", "gather")
GUARD_WORDS, GUARD = 256, 0x5A5AA5A5
_TORCH_TYPE = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
_RUNS = {}


def _launch(case, form):
    """One call of the entry on pre-filled outputs: (g_tokens, g_ref, prefill of each, guard intact)."""
    B, V, h, w, Cn, Q = (case[k] for k in ("B", "V", "h", "w", "C", "Q"))
    tok = torch.from_numpy(case["tokens"]).to(_TORCH_TYPE[case["tok_kind"]]).cuda().contiguous()
    assert np.array_equal(tok.float().cpu().numpy(), case["tokens"])                 # the oracle sees the widened values
    T = torch.from_numpy(case["T_cl"]).cuda().contiguous()
    assert T.dtype == torch.float64
    cam, ref, g = dev(case["camera"]), dev(case["ref"]), dev(case["g_tgt"])
    pre_t, pre_r = S.prefill((B, V * h * w, Cn), 1), S.prefill((B, Q, 3), 2)
    gt, gr = torch.from_numpy(pre_t).cuda(), torch.from_numpy(pre_r).cuda()
    scratch, sp, nbytes = None, None, 0
    if form == "gather":
        nbytes = lib().parq_k_project_sample_backward_scratch_bytes(B, V, Q)
        assert nbytes == B * Q * V * 8 * 4
        scratch = torch.full((nbytes // 4 + GUARD_WORDS,), GUARD, dtype=torch.int32, device="cuda")
        sp = C.c_void_p(scratch.data_ptr())
    _lib.check(lib().parq_k_project_sample_backward(_lib.token_ptr(tok), case["tok_type"], C.c_void_p(T.data_ptr()), _lib.ptr(cam),
                                                   _lib.ptr(ref), (C.c_float * 6)(*S.SCALE), B, V, h, w, Cn, Q, _lib.ptr(g), _lib.ptr(gt),
                                                   _lib.ptr(gr), sp, nbytes, sptr()), "project_sample_backward")
    torch.cuda.synchronize()
    # the guard intact, and the head of every (query, view) record written: the gather form is what ran
    guard_ok = scratch is None or bool((scratch[nbytes // 4:] == GUARD).all().item() and (scratch[:nbytes // 4:8] != GUARD).all().item())
    return gt.cpu().numpy(), gr.cpu().numpy(), pre_t, pre_r, guard_ok


def _run(cid, form):
    if (cid, form) not in _RUNS:
        _RUNS[cid, form] = _launch(S.make_case(cid), form)
    return _RUNS[cid, form]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _report(cid, form, what, err, bound, note=None):
    r = err / np.maximum(bound, 1e-300)
    ratio = float(r.max())
    print("sample_bwd ratio %-10s %-7s %-8s worst |err| / bound %.4f%s" % (cid, form, what, ratio, note(r) if note else ""))
    return ratio


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("cid", S.CASE_IDS)
def test_token_gradient_per_element(cid, form):
    """|got - want| <= (K + 6) 2^-23 sum|t_i| + ulp(prefill) for every element, the guard behind the scratch untouched, and every
    token row the oracle leaves at exactly zero bit-identical to its pre-fill (a masked corner written at its stand-in index 0 shows
    here)."""
    case, o, terms = S.reference(cid)
    got, _, pre, _, guard_ok = _run(cid, form)
    assert guard_ok
    err = np.abs(got.astype(np.float64) - (pre.astype(np.float64) + o["g_tokens"]))
    other = _run(cid, FORMS[1 - FORMS.index(form)])[0]
    note = lambda r: " (at an element with K = %d; %d of %d elements differ in bits from the other form)" % (
        terms["K"][np.unravel_index(r.argmax(), r.shape)[:2]], int((_bits(got) != _bits(other)).sum()), got.size)
    ratio = _report(cid, form, "g_tokens", err, S.token_bound(terms, pre), note)
    untouched = (o["g_tokens"] == 0).all(-1)
    assert untouched.any() and (~untouched).any()
    assert np.array_equal(_bits(got)[untouched], _bits(pre)[untouched])
    assert ratio <= 1.0


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("cid", S.CASE_IDS)
def test_coordinate_gradient_per_component(cid, form):
    """|got - want| <= (C / 64 + 14) 2^-23 sum_v (Su_v |du_v / dref_j| + Sv_v |dv_v / dref_j|) + ulp(prefill) for every component of
    every query outside the named exclusion; queries that no view samples add exactly 0.0."""
    case, o, terms = S.reference(cid)
    _, got, _, pre, _ = _run(cid, form)
    excluded = case["gref_excluded"]
    assert excluded.sum() == (14 if cid == "edges" else 0)
    err = np.abs(got.astype(np.float64) - (pre.astype(np.float64) + o["g_ref"]))
    bound = S.ref_bound(case, terms, o["jac"], pre)
    ratio = _report(cid, form, "g_ref", err[~excluded], bound[~excluded])
    silent = ~terms["on"].any(1) & ~excluded
    assert (o["g_ref"][silent] == 0).all() and np.array_equal(_bits(got)[silent], _bits(pre)[silent])
    if cid == "edges":
        fam = case["family"]
        assert silent[fam == "outside"].sum() == 4 and silent[fam == "clamp"].sum() == 3 and silent[fam == "camgrid"].sum() == 3
        assert (np.abs(o["g_ref"][(fam == "clamp") & ~excluded & ~silent]).max(-1) > 50).all()     # the 1 / zc gains are there
    assert np.isfinite(got).all() and ratio <= 1.0


@pytest.mark.parametrize("form", FORMS)
def test_lattice_contribution_is_exact(form):
    """A token whose only contribution is one query on its exact pixel (weight exactly 1) holds prefill + g_tgt * (1 / denom) in
    float32, bit for bit."""
    case, o, terms = S.reference("edges")
    got, _, pre, _, _ = _run("edges", form)
    units = S.unit_rows(case, o["p2d"], terms)
    assert len(units) == case["V"]
    for b, row, q in units:
        inv = np.float32(1.0) / np.float32(terms["denom"][b, q])
        want = pre[b, row] + case["g_tgt"][b, q] * inv
        assert want.dtype == np.float32 and np.array_equal(_bits(got[b, row]), _bits(want)), (b, row, q)


@pytest.mark.parametrize("cid", S.CASE_IDS)
def test_gather_form_repeats_bit_for_bit(cid):
    first = _run(cid, "gather")
    again = _launch(S.make_case(cid), "gather")
    assert again[4] and np.array_equal(_bits(first[0]), _bits(again[0])) and np.array_equal(_bits(first[1]), _bits(again[1]))


@pytest.mark.parametrize("cid", S.FP32_CASE_IDS)
def test_forward_per_row(cid):
    """parq_k_project_sample on the same cases, every query row against float64 within (4 V + 6) 2^-23 sum|terms|; rows that no view
    samples are exactly zero.  The forward entry takes float32 poses: the oracle gets the same rounded poses (the identity is exact)."""
    case = S.make_case(cid)
    B, V, h, w, Cn, Q = (case[k] for k in ("B", "V", "h", "w", "C", "Q"))
    T32 = case["T_cl"].astype(np.float32)
    c32 = dict(case, T_cl=T32.astype(np.float64))
    o = S.oracle(c32)
    terms = S.scatter_terms(c32, o["p2d"], o["valid"])
    assert np.array_equal(o["valid"], S.reference(cid)[1]["valid"])                   # the rounding of the poses flips no count
    tok, T, cam, ref = dev(case["tokens"]), dev(T32), dev(case["camera"]), dev(case["ref"])
    tgt = torch.from_numpy(S.prefill((B, Q, Cn), 3)).cuda()                          # the forward overwrites
    _lib.check(lib().parq_k_project_sample(_lib.ptr(tok), _lib.ptr(T), _lib.ptr(cam), _lib.ptr(ref), (C.c_float * 6)(*S.SCALE), B, V, h,
                                          w, Cn, Q, _lib.ptr(tgt), None, sptr()), "project_sample")
    torch.cuda.synchronize()
    got = tgt.cpu().numpy()
    ratio = _report(cid, "-", "forward", np.abs(got.astype(np.float64) - o["tgt"]), S.forward_bound(case, terms))
    silent = ~terms["on"].any(1)
    assert (got[silent] == 0).all() and (o["tgt"][silent] == 0).all() and (cid != "edges" or silent.sum() >= 10)
    assert ratio <= 1.0

"""CPU tier of the project-and-sample backward tests: the hand-placed cases of tests/sample_bwd_cases.py do what they say, and the
float64 oracle they are judged against (autograd of oracle.parq_oracle.project_and_sample) is itself checked — against central
differences, against the grid_sample form, and against the scatter spelled out term by term that supplies the error bounds.
Also the entry point parq_k_project_sample_backward: declared, typed, exported, and refusing what it must."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import sample_bwd_cases as S
from oracle import parq_oracle as O
from parq_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_edges_holds_every_family_and_the_exact_coordinates_are_exact():
    case, o, terms = S.reference("edges")
    fam, valid, on = case["family"], o["valid"], terms["on"]
    for f in S.FAMILIES:
        assert (fam == f).sum() >= 2, f
    assert valid.any() and (~valid).any()
    ex = case["exact"][0]
    assert ex.sum() == case["Q"] - 2                                   # all but the two clamped points that divide by eps
    for v in range(case["V"]):                                         # scene 0: identity views
        assert np.array_equal(o["p2d"][0, v][ex], case["intended"][0][ex])
    q = lambda f: np.nonzero(fam[0] == f)[0]
    assert valid[0][:, q("lattice")].all() and on[0][:, q("lattice")].all()
    assert on[0][0, q("band")].all() and not valid[0][0, q("band")].any() and not valid[0][2, q("band")].any()
    assert not valid[0][:, q("novalid")].any() and on[0][:, q("novalid")].all() and (terms["denom"][0, q("novalid")] == 1).all()
    cg = q("camgrid")
    assert valid[0][1, cg].all() and not valid[0][0, cg].any() and on[0][1, cg].any() and (~on[0][1, cg]).any()
    # what `outside` adds to the tokens is nothing: every weight it meets is exactly zero
    g0 = dict(case, g_tgt=np.where((fam == "outside")[..., None], case["g_tgt"], 0).astype(np.float32))
    assert (S.scatter_terms(g0, o["p2d"], valid)["abs"] == 0).all()
    cl = q("clamp")
    z = S.project(case["ref"], case["T_cl"], case["camera"])[1][0, 0, cl]
    assert (z > S.EPS).sum() == 2 and ((z > 0) & (z <= S.EPS)).sum() == 3 and (z < 0).sum() == 3
    assert on[0][0, cl[(z > 0)]].all() and not on[0][0, cl[z < 0]].any() and not valid[0][:, cl[z <= S.EPS]].any()
    assert np.abs(o["p2d"][0, 0, cl[z < 0]]).max() >= 1e6 and np.abs(o["p2d"][0, 0, cl[z < 0]]).max(-1).min() >= 1e3
    assert np.abs(o["jac"][0, 0, cl[z > S.EPS], 0, 0]).min() == 8 * 512                # the ~500 gains, times the scale box
    # the excluded set is the lattice, the exact -1 / w, and the clamp query on the principal point: its size is pinned
    assert case["gref_excluded"].sum() == 9 + 4 + 1 and not case["gref_excluded"][1].any()
    assert (fam == "lattice")[0].sum() == 9 and case["gref_excluded"][0][fam[0] == "lattice"].all()


def test_edges_leaves_stray_writes_somewhere_visible():
    """Token (0, 0) of a view is untouched, and masked corners' stand-in rows (index 0 in place of an out-of-range one) include rows
    that nothing touches: a corner written despite its mask lands where the bit comparison sees it."""
    case, o, terms = S.reference("edges")
    hw = case["h"] * case["w"]
    assert any(terms["K"][b, v * hw] == 0 and (terms["abs"][b, v * hw] == 0).all() for b in range(case["B"]) for v in range(case["V"]))
    stray_untouched = {(b, r) for b, r in terms["stray"] if terms["K"][b, r] == 0}
    units = S.unit_rows(case, o["p2d"], terms)                                         # the interior lattice point, alone on its token
    assert len(units) == case["V"] and all(b == 0 and terms["denom"][b, q] == 3 for b, _, q in units)
    band = {r % hw for b, r in stray_untouched if b == 0}                            # scene 0: the placed bands
    assert 3 * case["w"] in band and 2 in band, sorted(stray_untouched)                # tokens (3, 0) and (0, 2), in every view
    assert len(stray_untouched) >= 2 * case["V"] + 1, sorted(stray_untouched)


@pytest.mark.parametrize("cid", S.CASE_IDS)
def test_counts_do_not_depend_on_precision_and_margins_hold(cid):
    case, o, terms = S.reference(cid)
    p2d, z, valid = S.project(case["ref"], case["T_cl"], case["camera"])
    assert np.array_equal(valid, o["valid"]) and np.abs(p2d - o["p2d"]).max() <= 1e-12 * max(1.0, np.abs(p2d).max())
    t32 = lambda a: torch.from_numpy(np.asarray(a, np.float32))
    with torch.no_grad():
        _, _, valid32 = O.project_and_sample(t32(case["tokens"]), O.denormalize(t32(case["ref"]), S.SCALE), t32(case["T_cl"]),
                                             t32(case["camera"]), case["h"], case["w"], False)
    assert np.array_equal(valid32.numpy(), o["valid"])
    # margins: every (query, view) that is not exact by construction stays MARGIN off every lattice line and 1e-4 off the clamp;
    # exact ones that sample and whose coordinate gradient is judged stay off the lattice too
    dist = S.lattice_distance(o["p2d"])                                                # (B,V,Q)
    free = ~case["exact"][:, None, :] | (terms["on"] & ~case["gref_excluded"][:, None, :])
    assert (dist[free] >= S.MARGIN).all()
    assert (np.abs(z - S.EPS)[np.broadcast_to(~case["exact"][:, None, :], z.shape)] > 1e-4).all()
    assert valid.any() and (~valid).any() and terms["on"].any() and (~terms["on"]).any()
    if case["V"] > 1:                                                                  # the rotated views are not idle
        assert terms["on"][:, -1].mean() > 0.2 and valid[:, -1].mean() > 0.1


@pytest.mark.parametrize("cid", S.CASE_IDS)
def test_scatter_terms_are_the_autograd_gradient(cid):
    """The term-by-term scatter that supplies sum|t| and K is the same function as the autograd oracle, and leaves the same rows at
    exactly zero (so the float64 round trip through the normalised grid moved no lattice point across a pixel)."""
    case, o, terms = S.reference(cid)
    assert (np.abs(terms["g_tokens"] - o["g_tokens"]) <= 1e-13 * terms["abs"] + 1e-300).all()
    assert np.array_equal((terms["abs"] == 0).all(-1), (o["g_tokens"] == 0).all(-1))
    assert np.array_equal(terms["K"] == 0, (terms["abs"] == 0).all(-1))
    assert (np.abs(o["tgt"]) <= terms["fwd_abs"] * (1 + 1e-12) + S.ORACLE_NOISE).all()
    assert (o["tgt"][~terms["on"].any(1)] == 0).all()


def _loss_rows(case, ref):
    t = lambda a: torch.from_numpy(np.asarray(a)).double()
    with torch.no_grad():
        tgt, _, _ = O.project_and_sample(t(case["tokens"]), O.denormalize(torch.from_numpy(ref), S.SCALE), torch.from_numpy(case["T_cl"]),
                                         t(case["camera"]), case["h"], case["w"], False)
    return (tgt.numpy() * case["g_tgt"].astype(np.float64)).sum(-1)                    # (B,Q): a query's tgt row depends on its ref only


@pytest.mark.parametrize("cid", S.CASE_IDS)
def test_oracle_coordinate_gradient_against_central_differences_and_grid_sample(cid):
    case, o, terms = S.reference(cid)
    judged = ~case["gref_excluded"]
    z = S.project(case["ref"], case["T_cl"], case["camera"])[1]
    step = np.maximum(np.abs(z), 2.0 ** -11).min(1) * 2.0 ** -18 / 8                   # (B,Q) in ref units: 4e-6 of the depth
    px = np.abs(o["jac"]).max((-1, -2)) * step[:, None, :]                             # pixel displacement of the probe, (B,V,Q)
    assert (px[terms["on"]] < S.MARGIN / 2).all()                                      # no probe crosses a lattice line
    ref64 = case["ref"].astype(np.float64)
    scale = np.maximum(np.abs(o["g_ref"]).max(-1), 1e-300)
    for j in range(3):
        d = np.zeros_like(ref64)
        d[..., j] = step
        fd = (_loss_rows(case, ref64 + d) - _loss_rows(case, ref64 - d)) / (2 * step)
        err = np.abs(fd - o["g_ref"][..., j]) / scale
        assert err[judged].max() < 1e-6, (j, err[judged].max())
        assert (fd[judged & (o["g_ref"] == 0).all(-1)] == 0).all()
    gs = S.oracle(case, reference_ops=True)
    err = np.abs(gs["g_ref"] - o["g_ref"]).max(-1) / scale
    assert err[judged].max() < 1e-9, err[judged].max()
    assert (o["g_ref"][~terms["on"].any(1)] == 0).all()


def test_later_rounds_and_chunks_of_the_gather_are_entered():
    """Computed on the host from the cases: the second compaction round (queries 256..) of `seams` and the second list chunk
    (queries 1024..) of `chunks` have hits in every tile of the identity view, and all four waves of the first round do."""
    case, o, _ = S.reference("seams")
    assert case["Q"] > S.ROUND and (S.tile_hits(case, o["p2d"], S.ROUND)[:, 0] > 0).all()
    assert (S.wave_hits(case, o["p2d"])[:, 0] > 0).all()
    x0, y0, on = S.footprint(o["p2d"][:, 0], case["h"], case["w"])
    for xs in (7, 15):
        assert (on & (x0 == xs)).sum() >= 8
    assert (on & (y0 == 7)).sum() >= 8 and (on & (x0 == 15) & (y0 == 7)).sum() >= 2
    case, o, _ = S.reference("chunks")
    assert case["Q"] > S.CHUNK and (S.tile_hits(case, o["p2d"], S.CHUNK) > 0).all()
    for cid in ("edges", "views17", "wide", "tok16-f16"):
        assert S.SHAPES[cid][2] < S.TILE and S.SHAPES[cid][3] < S.TILE                # a view smaller than one gather tile


def test_case_statistics(capsys):
    """Q, tokens touched, worst K, hits of the later rounds / chunks — printed for the record (pytest -s)."""
    for cid in S.CASE_IDS:
        case, o, terms = S.reference(cid)
        r2 = S.tile_hits(case, o["p2d"], S.ROUND) if case["Q"] > S.ROUND else None
        c2 = S.tile_hits(case, o["p2d"], S.CHUNK) if case["Q"] > S.CHUNK else None
        with capsys.disabled():
            print("sample_bwd case %-10s Q %4d tokens touched %4d of %4d worst K %3d round-2 hits/tile %s chunk-2 hits/tile %s" % (
                cid, case["Q"], int((terms["K"] > 0).sum()), terms["K"].size, int(terms["K"].max()),
                "-" if r2 is None else "%d..%d" % (r2.min(), r2.max()), "-" if c2 is None else "%d..%d" % (c2.min(), c2.max())))
        assert (terms["K"] > 0).any() and (terms["K"] == 0).any()


def test_prefill_is_non_zero_and_small():
    p = S.prefill((7, 13), 3)
    assert p.dtype == np.float32 and (p != 0).all() and (p > 0).any() and (p < 0).any()
    assert (np.abs(p) >= 2.0 ** -10).all() and (np.abs(p) < 1.5 * 2.0 ** -10).all() and len(np.unique(p)) > 40


def test_header_binding_and_library_agree_on_the_entry_point():
    hdr = open(os.path.join(ROOT, "include", "parq_hip.h")).read()
    want = {"parq_k_project_sample_backward_scratch_bytes": ["B", "V", "Q"],
            "parq_k_project_sample_backward": ["tokens", "token_type", "T_camera_local", "camera", "ref", "scale6_host", "B", "V", "hh",
                                               "ww", "C", "Q", "g_tgt", "g_tokens", "g_ref", "det_scratch", "det_scratch_bytes", "stream"]}
    api = open(os.path.join(ROOT, "parq_amd", "csrc", "api.hip")).read()
    for name, names in want.items():
        m = re.search(r"\b(?:int|size_t)\s+\(%s\)\s*\(([^;]*)\)\s*;" % name, hdr)
        assert m, "include/parq_hip.h must declare %s with a parenthesised name" % name
        params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
        assert [p.split()[-1].lstrip("*") for p in params] == names, name
        res, args = _lib.EXTRA_SYMBOLS[name]
        assert name not in _lib.SYMBOLS and len(args) == len(names) and res is (C.c_size_t if name.endswith("bytes") else C.c_int)
        d = re.search(r"\b(?:int|size_t)\s+%s\s*\(([^)]*)\)\s*\{" % name, api)
        assert d, "parq_amd/csrc/api.hip must define %s" % name
        types = lambda s: [re.sub(r"\s+", " ", re.sub(r"\w+$", "", p.strip()).replace(" *", "*")).strip() for p in s.replace("\n", " ").split(",")]
        assert types(d.group(1)) == types(m.group(1)), name
    res, args = _lib.EXTRA_SYMBOLS["parq_k_project_sample_backward"]
    assert args[1] is C.c_int32 and args[5] == C.POINTER(C.c_float) and args[16] is C.c_size_t and args[6:12] == [C.c_int32] * 6
    lib = _lib.load()
    for name in want:
        fn = getattr(lib, name)
        assert fn.argtypes == _lib.EXTRA_SYMBOLS[name][1] and fn.restype is _lib.EXTRA_SYMBOLS[name][0]
    assert lib.parq_k_project_sample_backward_scratch_bytes(2, 3, 48) == 2 * 3 * 48 * 8 * 4
    assert lib.parq_k_project_sample_backward_scratch_bytes(0, 3, 48) == 0


def test_entry_point_refuses_bad_arguments_before_any_launch():
    """Every refusal below returns ahead of the first HIP call, so none of the (host) pointers is ever read."""
    lib = _lib.load()
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    sc = (C.c_float * 6)(*S.SCALE)
    call = lambda tok=p, tt=0, B=1, V=2, hh=5, ww=6, Cn=64, Q=4, g=p, scratch=None, nbytes=0: lib.parq_k_project_sample_backward(
        tok, tt, p, p, p, sc, B, V, hh, ww, Cn, Q, g, p, p, scratch, nbytes, None)
    need = lib.parq_k_project_sample_backward_scratch_bytes(1, 2, 4)
    for kw in (dict(tok=None), dict(g=None), dict(tt=3), dict(tt=-1), dict(B=0), dict(V=0), dict(hh=1), dict(ww=1), dict(Q=0), dict(Cn=66),
               dict(Cn=1028), dict(scratch=p, nbytes=need - 1), dict(scratch=p, nbytes=0), dict(scratch=None, nbytes=need)):
        assert call(**kw) == 1, kw                                                     # PARQ_ERR_ARG
        assert lib.parq_last_error()

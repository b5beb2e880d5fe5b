"""GPU tier: parq_parse_pred (parq_amd/csrc/postproc.hip: boxes, validity window, greedy 3-D NMS, one workgroup per scene) against the
float64 oracle of tests/tail_oracles.py, which tests/test_tail_oracles_cpu.py pins to the reference's golden g11.  Every loop of the
kernel strides by its 256 threads; the shapes here take a second, third and fourth trip round each of them (Q up to the limit of
1024) and stand on both sides of 256 and 1024."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from parq_amd import _lib, synth
from gpu_util import dev, lib, sptr
from parse_pred_cases import (GENERIC_CASES, GENERIC_TRACK_SCALE, NCLS, TRACK_SCALE, generic_inputs, lattice_case)
from tail_oracles import parse_pred_oracle

pytestmark = pytest.mark.gpu


def run_kernel(x, track_scale, for_vis, enable_nms=1, ncls=None):
    B, Q = x["center"].shape[:2]
    d = {k: dev(v) for k, v in x.items()}
    obbs = torch.full((B, Q, 19), -77.0, device="cuda")
    mask = torch.full((B, Q), 7, dtype=torch.uint8, device="cuda")
    ts = (C.c_float * 6)(*[float(t) for t in track_scale])
    _lib.check(lib().parq_parse_pred(_lib.ptr(d["center"]), _lib.ptr(d["size"]), _lib.ptr(d["rot6"]), _lib.ptr(d["prob"]), B, Q,
                                     ncls or x["prob"].shape[-1], ts, for_vis, enable_nms, _lib.ptr(obbs), C.c_void_p(mask.data_ptr()),
                                     sptr()), "parse_pred")
    m = mask.cpu().numpy()
    assert set(np.unique(m).tolist()) <= {0, 1}
    return obbs.cpu().numpy(), m.astype(bool)


@functools.lru_cache(maxsize=None)
def _lattice(Q, B):
    x, notes, kinds = lattice_case(Q, B)
    return x, notes, kinds, {v: parse_pred_oracle(x["center"], x["size"], x["rot6"], x["prob"], TRACK_SCALE, v, 1) for v in (0, 1)}


@pytest.mark.parametrize("for_vis", [0, 1])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("Q", [1, 2, 255, 256, 257, 512, 1024])
def test_lattice_inputs_are_reproduced_bit_for_bit(Q, B, for_vis):
    """Inputs on which every float32 operation of the kernel is exact (tests/parse_pred_cases.py): the boxes equal the float64 oracle's
    bit for bit and the mask equals it for every query, nothing excluded.  The edge cases sit in scene 0 of every Q >= 255: an IoU
    exactly on 0.1 and on 0.2 (kept: the comparison is strict) and one grid point above, an IoU between the double threshold and the
    float one (suppressed), tied scores, tied class probabilities, background tied with a class, centres on the window, boxes of zero
    size, nested boxes, identical boxes of two classes.  With B = 3, scene 1 has no candidate and scene 2 has one."""
    x, notes, kinds, want = _lattice(Q, B)
    w = want[for_vis]
    obbs, mask = run_kernel(x, TRACK_SCALE, for_vis)
    w32 = w.obbs.astype(np.float32)
    assert np.array_equal(w32.astype(np.float64), w.obbs)                   # the oracle's boxes are float32 numbers
    assert np.array_equal(obbs.view(np.uint32), w32.view(np.uint32)), np.argwhere(obbs.view(np.uint32) != w32.view(np.uint32))[:5]
    assert np.array_equal(mask, w.mask), np.argwhere(mask != w.mask)[:10]
    for b, kind in enumerate(kinds):
        cand, kept = int((w.label[b] != NCLS - 1).sum()), int(mask[b].sum())
        assert cand == {"background": 0, "single": 1}.get(kind, cand)
        assert (0 < kept < cand) if cand > 1 else kept == cand            # a single candidate is its own survivor
    if kinds[0] == "full":
        at = lambda note: [bool(mask[0, i]) for i in notes[note]]
        # what the edge cases must come to, stated here and not only through the oracle
        assert at("iou_on_0.1") == [True, True]
        assert at("iou_above_0.1") == [True, bool(for_vis)]
        assert at("iou_on_0.2") == [True, bool(for_vis)]
        assert at("iou_above_0.2") == [True, False]
        assert at("gap_0.1") == [True, bool(for_vis)]
        assert at("gap_0.2") == [True, False]
        i, j = notes["tie_overlap"]
        assert mask[0, max(i, j)] and not mask[0, min(i, j)]
        assert at("tie_apart") == [True, True]
        assert at("class_tie") == [True, bool(for_vis), False] and w.label[0, notes["class_tie"][0]] == 2
        assert at("background_tie") == [True, True] and at("background_top") == [False]
        assert [int(w.label[0, i]) for i in notes["background_tie"]] == [3, 0]
        assert all(at("zero_size"))
        assert at("contains") == [True, False, True, True]
        assert at("other_class") == [True, bool(for_vis)]
        assert at("on_window") == [bool(for_vis)] * 4 and all(at("inside_window"))


@functools.lru_cache(maxsize=None)
def _generic(seed, Q, anchors, nan_rows=()):
    x = generic_inputs(seed, 2, Q, anchors)
    for b, q in nan_rows:
        for v in x.values():
            v[b, q] = np.nan
    return x, {v: parse_pred_oracle(x["center"], x["size"], x["rot6"], x["prob"], GENERIC_TRACK_SCALE, v, 1) for v in (0, 1)}


# 200 anchors at Q = 1024: some 27 boxes per scene survive in the evaluation variant and 320 in the visualisation variant, pick after
# pick.  Seed chosen on the CPU like the others (51 .. 57 fall under 6e-5): the float64 oracle's smallest |IoU - threshold| is
# 1.5e-4 (evaluation) / 9.2e-5 (visualisation).
MANY_PICKS = (50, 1024, 200)


@pytest.mark.parametrize("for_vis", [0, 1])
@pytest.mark.parametrize("seed,Q,anchors", GENERIC_CASES + [MANY_PICKS])
def test_random_rotations_match_the_oracle_for_every_query(seed, Q, anchors, for_vis):
    """The golden's generator at Q = 257, 512, 1024 (and with 200 anchors, where many picks follow each other): boxes within 2e-6,
    masks equal for every query.  Condition, from the oracle alone: no evaluated IoU within 2e-5 of the threshold (the float32 bounds
    carry about 1e-6 of IoU error at these sizes); scores need none, they are read, not computed."""
    x, want = _generic(seed, Q, anchors)
    w = want[for_vis]
    print("seed %d Q %d anchors %d for_vis %d: margin %.2e over %d pairs, kept %d" % (seed, Q, anchors, for_vis, w.margin, w.pairs, w.mask.sum()))
    assert w.margin >= 2e-5 and w.pairs > Q
    obbs, mask = run_kernel(x, GENERIC_TRACK_SCALE, for_vis)
    err = np.abs(obbs - w.obbs).max()
    print("box error %.2e" % err)
    assert err < 2e-6
    assert np.array_equal(mask, w.mask), np.argwhere(mask != w.mask)[:10]
    assert 0 < mask.sum() < (w.label != NCLS - 1).sum()
    if anchors > 100:
        assert min(len(np.nonzero(m)[0]) for m in want[1].mask) > 100


NMS_OFF = (42, 300, 12)


def test_without_nms_the_mask_is_the_validity_window():
    x, _ = _generic(*NMS_OFF)
    c = x["center"].astype(np.float64)
    ts = GENERIC_TRACK_SCALE
    valid = (c[..., 0] > ts[0]) & (c[..., 0] < ts[1]) & (c[..., 2] > ts[4]) & (c[..., 2] < ts[5])
    assert valid.any() and not valid.all()
    for for_vis in (0, 1):
        w = parse_pred_oracle(x["center"], x["size"], x["rot6"], x["prob"], ts, for_vis, 0)
        obbs, mask = run_kernel(x, ts, for_vis, enable_nms=0)
        assert np.array_equal(mask, w.mask)
        assert np.array_equal(mask, np.ones_like(valid) if for_vis else valid)
        assert np.abs(obbs - w.obbs).max() < 2e-6


NAN_ROWS = ((0, 3), (0, 140), (0, 256), (0, 299), (1, 0), (1, 257))


@pytest.mark.parametrize("for_vis", [0, 1])
def test_nan_rows_are_visited_first_and_leave_every_other_query_alone(for_vis):
    """A few query rows NaN in all four inputs (a decoder row that went NaN under the "off" range policy).  The ranking is a total
    order: a NaN score ranks above every number, so those boxes are visited first and picked (np.argsort puts NaN last), their IoU
    with anything is not above the threshold, and every other query's box and mask bit are the oracle's.  A NaN centre fails the
    window: 0 in the evaluation variant, 1 in the visualisation variant."""
    x, want = _generic(NMS_OFF[0], 300, 12, NAN_ROWS)
    w = want[for_vis]
    print("margin %.2e over %d pairs" % (w.margin, w.pairs))
    assert w.margin >= 2e-5
    obbs, mask = run_kernel(x, GENERIC_TRACK_SCALE, for_vis)
    obbs2, mask2 = run_kernel(x, GENERIC_TRACK_SCALE, for_vis)
    assert np.array_equal(mask, w.mask), np.argwhere(mask != w.mask)[:10]
    nan = np.zeros(mask.shape, bool)
    nan[tuple(np.array(NAN_ROWS).T)] = True
    assert (mask[nan] == bool(for_vis)).all()
    assert np.isnan(w.obbs[nan][:, 6:18]).all() and np.isfinite(w.obbs[~nan]).all()
    assert np.abs(obbs[~nan] - w.obbs[~nan]).max() < 2e-6
    assert np.allclose(obbs[nan], w.obbs[nan], rtol=0, atol=2e-6, equal_nan=True)
    assert obbs.tobytes() == obbs2.tobytes() and mask.tobytes() == mask2.tobytes()
    assert 0 < mask[~nan].sum() < (~nan).sum()


def test_bad_arguments_are_refused_with_a_message():
    l = lib()
    t = torch.zeros(2 * 1025 * 19, device="cuda")
    m = torch.zeros(2 * 1025, dtype=torch.uint8, device="cuda")
    ts = (C.c_float * 6)(*TRACK_SCALE)
    for B, Q, ncls in ((1, 1025, 10), (1, 0, 10), (0, 16, 10), (1, 16, 1)):
        rc = l.parq_parse_pred(_lib.ptr(t), _lib.ptr(t), _lib.ptr(t), _lib.ptr(t), B, Q, ncls, ts, 0, 1, _lib.ptr(t), C.c_void_p(m.data_ptr()), sptr())
        assert rc == 1, (B, Q, ncls, rc)                        # PARQ_ERR_ARG
        assert len(l.parq_last_error()) > 0
    torch.cuda.synchronize()
    assert not t.any() and not m.any()                         # nothing was launched


@pytest.mark.parametrize("for_vis", [False, True])
def test_decoder_parse_pred_equals_the_direct_call_at_512_queries(for_vis):
    from parq_amd.decoder import PARQDecoder
    from parq_amd.wrappers import raw
    seed, Q, anchors = GENERIC_CASES[1]
    x, _ = _generic(seed, Q, anchors)
    cfg = synth.decoder_cfg(dim=64, queries=Q, heads=1, ffn=64, layers=1)
    cfg.TRACK_SCALE = GENERIC_TRACK_SCALE
    dec = PARQDecoder(cfg).cuda().eval()
    dec.for_vis = for_vis
    assert dec.enable_nms and dec.num_semcls + 1 == NCLS
    out = dec.parse_pred([{"center_unnormalized": dev(x["center"]), "size_unnormalized": dev(x["size"]), "ortho6d": dev(x["rot6"]),
                           "sem_cls_prob": dev(x["prob"])}])
    obbs, mask = run_kernel(x, GENERIC_TRACK_SCALE, int(for_vis))
    assert out["pred_mask"].dtype == torch.bool and out["pred_mask"].shape == (2, Q)
    assert np.array_equal(out["pred_mask"].cpu().numpy(), mask)
    assert raw(out["obbs_pred"]).cpu().numpy().tobytes() == obbs.tobytes()

"""GPU tier: the tracker's oriented-box IoU on the device (csrc/obb_iou.hip, parq_obb_iou) against the reference's values
(tests/golden/g12_f1.npz) and the host routine (parq_amd/f1_eval.py iou3d), through ctypes and through F1Calculator /
PARQDecoder.  The bound is the host routine's own against the reference (test_eval_cpu.py): 1e-12."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import eval_iou_cases as E
from gpu_util import lib
from oracle.make_golden import F1_CASE
from parq_amd import Pose, _lib, synth
from parq_amd.f1_eval import DeviceIoU, F1Calculator, canonical, host_iou_backend, iou3d, pack_segments

pytestmark = pytest.mark.gpu

TOL = 1e-12


def device_iou(segments):
    """(3-D, footprint) matrices of the segments from one parq_obb_iou call through the Python wrapper."""
    return DeviceIoU("cuda")(segments, footprint=True)


def host_both(A, B):
    m = np.array([[iou3d(a, b) for b in B] for a in A], np.float64).reshape(len(A), len(B), 2)
    return m[..., 0], m[..., 1]


def assert_same(got, want, what):
    """Within 1e-12 everywhere, NaN where the host has NaN, and exactly zero where the host is exactly zero."""
    assert got.shape == want.shape, what
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    ok = ~np.isnan(want)
    err = float(np.abs(got[ok] - want[ok]).max()) if ok.any() else 0.0
    print("%s: %d values, %d non-zero, max |device - host| = %.3e" % (what, want.size, int((want[ok] != 0).sum()), err))
    assert err < TOL, (what, err)
    assert np.array_equal(got[ok] == 0, want[ok] == 0), what


def test_reference_values_and_degenerate_boxes():
    g = E.g12()
    pairs = g["iou_pairs"]
    assert len(pairs) == 24
    # 24 segments of one pair each, raw ctypes call
    A = np.stack([canonical(p[0]) for p in pairs])
    B = np.stack([canonical(p[1]) for p in pairs])
    buf, (oa, ob, ot), na, nb, table, total = pack_segments([(A[k:k + 1], B[k:k + 1]) for k in range(24)])
    dev = torch.from_numpy(buf).cuda()
    out = torch.full((2, total), -1.0, dtype=torch.float64, device="cuda")
    p = lambda off: C.c_void_p(dev.data_ptr() + 8 * off)
    _lib.check(lib().parq_obb_iou(p(oa), na, p(ob), nb, p(ot), 24, total, C.c_void_p(out[0].data_ptr()), C.c_void_p(out[1].data_ptr()),
                                  _lib.stream_ptr()), "parq_obb_iou")
    got = out.cpu().numpy().T
    print("g12 pairs: max |device - reference| = %.3e" % float(np.abs(got - g["iou_values"]).max()))
    assert np.abs(got - g["iou_values"]).max() < TOL
    # footprint output is optional
    out3 = torch.full((total,), -1.0, dtype=torch.float64, device="cuda")
    _lib.check(lib().parq_obb_iou(p(oa), na, p(ob), nb, p(ot), 24, total, C.c_void_p(out3.data_ptr()), None, _lib.stream_ptr()), "parq_obb_iou")
    assert torch.equal(out3, out[0])
    # far apart, NaN, and the box standing on edge of test_eval_cpu.py
    box = canonical(pairs[0][0])
    far = canonical(pairs[0][0] + 50.0)
    edge_on = canonical(pairs[0][0][:, [0, 2, 1]])
    m3, m2 = device_iou([(box[None], far[None]), ((box * np.nan)[None], far[None]), (far[None], (box * np.nan)[None]),
                         (edge_on[None], edge_on[None])])
    for k in range(3):
        assert m3[k][0, 0] == 0.0 and m2[k][0, 0] == 0.0, k
    assert m3[3][0, 0] == 0.0
    want = iou3d(edge_on, edge_on)
    assert np.isnan(m2[3][0, 0]) == np.isnan(want[1]) and (np.isnan(want[1]) or abs(m2[3][0, 0] - want[1]) < TOL)


def test_arguments_and_empty_launches():
    l = lib()
    box = torch.from_numpy(E.random_boxes(2, 1)).cuda()
    out = torch.full((4,), -1.0, dtype=torch.float64, device="cuda")
    table = torch.tensor([[0, 2, 0, 0, 0], [0, 0, 0, 2, 0]], dtype=torch.int64, device="cuda")
    bp, op, tp, sp = C.c_void_p(box.data_ptr()), C.c_void_p(out.data_ptr()), C.c_void_p(table.data_ptr()), _lib.stream_ptr()
    assert l.parq_obb_iou(None, 0, None, 0, None, 0, 0, None, None, sp) == 0                    # S = 0
    assert l.parq_obb_iou(bp, 2, bp, 2, tp, 2, 0, op, None, sp) == 0                            # empty segments only
    torch.cuda.synchronize()
    assert bool((out == -1.0).all())
    assert l.parq_obb_iou(bp, 2, bp, 2, tp, -1, 0, op, None, sp) == 1                           # PARQ_ERR_ARG
    assert l.parq_obb_iou(bp, 2, bp, 2, tp, 1, -4, op, None, sp) == 1
    assert l.parq_obb_iou(bp, 2, bp, 2, tp, 1, 4, None, None, sp) == 1
    assert l.parq_obb_iou(None, 2, bp, 2, tp, 1, 4, op, None, sp) == 1
    assert l.parq_obb_iou(bp, 2, bp, 2, None, 1, 4, op, None, sp) == 1
    assert b"parq_obb_iou" in l.parq_last_error()
    # a table row that reaches outside the box arrays writes nothing
    bad = torch.tensor([[1, 2, 0, 2, 0]], dtype=torch.int64, device="cuda")
    assert l.parq_obb_iou(bp, 2, bp, 2, C.c_void_p(bad.data_ptr()), 1, 4, op, None, sp) == 0
    torch.cuda.synchronize()
    assert bool((out == -1.0).all())
    assert DeviceIoU("cuda")([]) == [] and DeviceIoU("cuda").launches == 0


def test_device_matches_host_on_random_boxes():
    """2071 pairs in five segments of different sizes (two of them empty) in one launch: 33 workgroups of 64 lanes, the last one
    partly filled, segment borders inside a workgroup.  Then every box against itself and against a copy shifted by 1e-3 along
    the world's (1, 1, 1) (the ground-truth jitter's shape), as 2 x 102 segments of one pair: there every inside test is a
    rounding-sign question."""
    A = E.random_boxes(63, 21)
    B = E.random_boxes(102, 22)
    cuts = [((0, 20), (0, 30)), ((20, 20), (30, 35)), ((20, 51), (35, 68)), ((51, 58), (38, 102)), ((58, 63), (50, 50))]
    segments = [(A[a0:a1], B[b0:b1]) for (a0, a1), (b0, b1) in cuts]
    assert sum(len(a) * len(b) for a, b in segments) == 600 + 0 + 1023 + 448 + 0
    backend = DeviceIoU("cuda")
    m3, m2 = backend(segments, footprint=True)
    assert backend.launches == 1 and backend.pairs == 2071
    want = [host_both(a, b) for a, b in segments]
    got3, got2 = np.concatenate([m.reshape(-1) for m in m3]), np.concatenate([m.reshape(-1) for m in m2])
    want3, want2 = np.concatenate([w[0].reshape(-1) for w in want]), np.concatenate([w[1].reshape(-1) for w in want])
    assert [m.shape for m in m3] == [(20, 30), (0, 5), (31, 33), (7, 64), (5, 0)]
    assert (want3 > 0.05).sum() > 200 and (want3 == 0).sum() > 1000         # the case has overlaps and misses
    assert_same(got3, want3, "random 3-D")
    assert_same(got2, want2, "random footprint")

    shifted = B + 1e-3 * np.array([1.0, -1.0, 1.0])               # world (1, 1, 1) in the canonical frame (x, -z, y)
    segments = [(B[k:k + 1], B[k:k + 1]) for k in range(len(B))] + [(B[k:k + 1], shifted[k:k + 1]) for k in range(len(B))]
    m3, m2 = backend(segments, footprint=True)
    assert backend.launches == 2
    want = [iou3d(a[0], b[0]) for a, b in segments]
    assert_same(np.array([m[0, 0] for m in m3]), np.array([w[0] for w in want]), "self / shifted 3-D")
    assert_same(np.array([m[0, 0] for m in m2]), np.array([w[1] for w in want]), "self / shifted footprint")


def test_tracker_run_on_device_matches_reference():
    rec = E.Recording(None)
    calc = F1Calculator(F1_CASE["conf"], iou_device="cuda")
    assert isinstance(calc.iou_backend, DeviceIoU)
    dev_backend = calc.iou_backend
    rec.inner = dev_backend
    calc.iou_backend = rec
    launches = []
    metrics = E.run_g12(calc, after_step=lambda k: launches.append(dev_backend.launches))
    E.assert_g12(calc, metrics)
    assert launches == [0, 1, 2, 3] and dev_backend.launches == 4         # one per step that associates, one for the metrics
    assert dev_backend.pairs == sum(sum(m.size for m in mats) for _, mats in rec.calls) > 4000
    worst = 0.0
    for segments, mats in rec.calls:
        for got, want in zip(mats, host_iou_backend(segments)):
            worst = max(worst, float(np.abs(got - want).max()) if got.size else 0.0)
            assert np.array_equal(got.astype(np.float32), want.astype(np.float32))
    print("g12 run: max |device - host| over %d pairs = %.3e" % (dev_backend.pairs, worst))
    assert worst < TOL


def test_duplicate_scene_name_on_device():
    steps = E.duplicate_name_steps()
    want = E.run_steps(E.host_calculator(), steps)
    calc = E.run_steps(F1Calculator(F1_CASE["conf"], iou_device="cuda"), steps)
    assert E.tracker_state(calc) == E.tracker_state(want)
    assert calc.iou_backend.launches == 1 + 3                              # one launch per wave that has tracks to meet
    assert calc.compute_metrics() == want.compute_metrics() and calc.iou_backend.launches == 5


def test_decoder_metrics_on_device():
    """The g11 scenario of test_gpu_decoder.test_update_metrics_drives_the_f1_trackers: the same outputs fed twice, so every track
    meets an identical box."""
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "oracle"))
    from make_golden import PARSE_CASE, parse_case_inputs
    from parq_amd import Obb3D
    from parq_amd.decoder import PARQDecoder
    x = parse_case_inputs(PARSE_CASE)
    B, Q = PARSE_CASE["B"], PARSE_CASE["Q"]
    cfg = synth.decoder_cfg(dim=64, queries=Q, heads=1, ffn=64, layers=1)
    cfg.TRACK_SCALE = PARSE_CASE["track_scale"]
    assert PARQDecoder.metrics_on_device is False
    dec = PARQDecoder(cfg).cuda().eval()
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    outs = [{"center_unnormalized": to(x["center"]), "size_unnormalized": to(x["size"]), "ortho6d": to(x["rot6"]),
             "sem_cls_prob": to(x["prob"])}]
    gt, _ = synth.make_boxes(77, B, 6, max_box=10)
    _, _, _, T_wl = synth.make_geometry(78, B, 2, 8, 10)
    names = ["room0", "room1"]
    results = {}
    for on_device in (False, True):
        dec.metrics_on_device = on_device
        np.random.seed(11)
        dec.reset_metrics()
        calc = dec.metrics_calculator[0]
        dec.update_metrics(outs, Obb3D(to(gt)), Pose(to(T_wl)), names)
        assert (calc.iou_backend is not None) == on_device
        first = calc.iou_backend.launches if on_device else 0
        dec.update_metrics(outs, Obb3D(to(gt)), Pose(to(T_wl)), names)
        metrics = dec.compute_metrics()
        if on_device:
            assert (first, calc.iou_backend.launches) == (0, 2)
        results[on_device] = (metrics, E.tracker_state(calc))
    assert results[True] == results[False]
    assert min(len(t) for t in results[True][1][0].values()) > 3
    dec.metrics_on_device = False
    assert dec.compute_metrics() == results[False][0] and dec.metrics_calculator[0].iou_backend is None

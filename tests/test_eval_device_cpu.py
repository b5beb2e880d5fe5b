"""CPU tier: the batched path of the F1 tracker (parq_amd/f1_eval.py: segments -> one IoU call per wave -> the unchanged
association per scene) with the host ``iou3d`` injected as its IoU source.  The device source is tests/test_gpu_eval_iou.py."""
import numpy as np
import pytest

import eval_iou_cases as E
from oracle.make_golden import F1_CASE
from parq_amd import f1_eval
from parq_amd.f1_eval import F1Calculator, host_iou_backend, pack_segments, split_matrices


def test_batched_path_reproduces_the_reference_run():
    rec = E.Recording(host_iou_backend)
    calc = F1Calculator(F1_CASE["conf"], iou_backend=rec)
    calls_after = []
    metrics = E.run_g12(calc, after_step=lambda k: calls_after.append(len(rec.calls)))
    E.assert_g12(calc, metrics)
    # snippet 0 creates every scene (nothing to associate); afterwards one call per step, and one for all three thresholds
    assert calls_after == [0, 1, 2, 3] and len(rec.calls) == 4
    # a step's call holds predictions and ground truth of every scene of the batch (2, 3, 2 scenes), the last one every scene
    assert [len(s) for s, _ in rec.calls] == [4, 6, 4, 3]
    host = E.run_g12(E.host_calculator())
    assert host == metrics


def test_duplicate_scene_name_is_processed_in_waves():
    steps = E.duplicate_name_steps()
    want = E.tracker_state(E.run_steps(E.host_calculator(), steps))
    rec = E.Recording(host_iou_backend)
    calc = E.run_steps(F1Calculator(F1_CASE["conf"], iou_backend=rec), steps)
    assert E.tracker_state(calc) == want
    assert set(calc.preds) == {"scene_a", "scene_b"} and len(calc.preds["scene_a"]) > len(calc.preds["scene_b"])
    # batch 1: scene_a's second entry waits for its first (1 call); batch 2: three entries of scene_a, three waves
    assert len(rec.calls) == 1 + 3
    assert [len(s) for s, _ in rec.calls] == [2, 2, 2, 2]          # each wave: scene_a's predictions and its ground truth
    assert calc.compute_metrics() == E.run_steps(E.host_calculator(), steps).compute_metrics()


def test_empty_detections_and_tracks():
    def outputs(keep):
        rng = np.random.RandomState(3)
        corners = np.stack([E._yaw_box_corners(rng.uniform(-1, 1, 3), rng.uniform(0.3, 0.6, 3), 0.3) for _ in range(4)])[None]
        prob = np.full((1, 4, 10), 0.05, np.float32)
        prob[..., 2] = 0.55
        return {"pred_corners_world": corners.astype(np.float32), "sem_cls_prob": prob, "pred_mask": np.full((1, 4), keep),
                "scene_name": ["s"]}
    gt_none = [{"labels": np.zeros((0,), np.int64), "gt_corners_world": np.zeros((0, 8, 3), np.float32)}]
    gt_some = [{"labels": np.array([2, 2]), "gt_corners_world": outputs(True)["pred_corners_world"][0, :2]}]
    seq = [(False, gt_none), (False, gt_none), (True, gt_some), (False, gt_none), (True, gt_some)]   # 0x0, 0x0, nx0, 0xn, nxn
    rec = E.Recording(host_iou_backend)
    got, want = F1Calculator(0.1, iou_backend=rec), F1Calculator(0.1)
    for calc in (got, want):
        np.random.seed(5)
        for keep, gt in seq:
            calc.step(outputs(keep), gt)
    assert E.tracker_state(got) == E.tracker_state(want) and len(got.preds["s"]) >= 4 and len(got.gts["s"]) >= 2
    shapes = [[m.shape for m in mats] for _, mats in rec.calls]
    assert shapes == [[(0, 0), (0, 0)], [(4, 0), (2, 0)], [(0, 4), (0, 2)], [(4, 4), (2, 2)]]
    assert got.compute_metrics() == want.compute_metrics()
    empty = F1Calculator(0.1, iou_backend=rec)
    assert all(v == 0 for v in empty.compute_metrics().values())   # no scene at all: no call
    assert len(rec.calls) == 4 + 1


def test_packing_layout():
    A = [np.arange(n * 24, dtype=np.float64).reshape(n, 8, 3) for n in (2, 0, 3)]
    B = [100 + np.arange(n * 24, dtype=np.float64).reshape(n, 8, 3) for n in (3, 5, 0)]
    buf, (oa, ob, ot), na, nb, table, total = pack_segments(list(zip(A, B)))
    assert (na, nb, total) == (5, 8, 6) and (oa, ob, ot) == (0, 5 * 24, 13 * 24) and buf.dtype == np.float64
    assert table.tolist() == [[0, 2, 0, 3, 0], [2, 0, 3, 5, 6], [2, 3, 8, 0, 6]]
    assert np.array_equal(buf[:ob], np.concatenate(A).reshape(-1)) and np.array_equal(buf[ob:ot], np.concatenate(B).reshape(-1))
    assert np.array_equal(buf[ot:].view(np.int64).reshape(3, 5), table)
    mats = split_matrices(np.arange(6.0), table)
    assert [m.shape for m in mats] == [(2, 3), (0, 5), (3, 0)] and mats[0].tolist() == [[0, 1, 2], [3, 4, 5]]
    assert pack_segments([])[-1] == 0 and pack_segments([])[0].size == 0


def test_default_stays_on_the_host_loop(monkeypatch):
    with pytest.raises(ValueError):
        F1Calculator(0.1, iou_device="cpu")                        # the option names a GPU; the host loop is None
    calc = F1Calculator(F1_CASE["conf"])
    assert calc.iou_device is None and calc.iou_backend is None
    filled = []
    host_matrix = f1_eval._iou_matrix
    monkeypatch.setattr(f1_eval, "_iou_matrix", lambda d, t: filled.append((len(d), len(t))) or host_matrix(d, t))
    monkeypatch.setattr(f1_eval, "host_iou_backend", None)
    monkeypatch.setattr(f1_eval, "DeviceIoU", None)
    steps = E.duplicate_name_steps()
    E.run_steps(calc, steps)
    assert len(filled) == 2 * (1 + 3)                              # predictions and ground truth of every revisit, pair by pair

"""Shared inputs of the batched / device oriented-box IoU tests (test_eval_device_cpu.py, test_gpu_eval_iou.py): the g12 tracker
run, a batch that names one scene twice, seeded random boxes, and a backend wrapper that records what the calculator asked for."""
import os

import numpy as np
import torch

import golden_util as G
from oracle.make_golden import F1_CASE, _yaw_box_corners, f1_case_inputs
from parq_amd.f1_eval import F1Calculator, canonical


def g12():
    return np.load(os.path.join(G.GOLDEN_DIR, "g12_f1.npz"))


def _feed(calc, st):
    out = {"pred_corners_world": torch.from_numpy(st["corners"]), "sem_cls_prob": torch.from_numpy(st["prob"]),
           "pred_mask": torch.from_numpy(st["mask"]), "scene_name": st["scenes"]}
    calc.step(out, [{"labels": torch.from_numpy(x["labels"]), "gt_corners_world": torch.from_numpy(x["corners"])} for x in st["gts"]])


def run_g12(calc, after_step=None):
    """The tracker run of test_eval_cpu.test_f1_tracker_matches_reference_run on `calc`; returns its metrics."""
    np.random.seed(F1_CASE["np_seed"])
    for k, st in enumerate(f1_case_inputs(F1_CASE)):
        _feed(calc, st)
        if after_step is not None:
            after_step(k)
    return calc.compute_metrics()


def assert_g12(calc, metrics):
    """Track counts, classes, ids, scores and the nine metrics identical to the reference's (tests/golden/g12_f1.npz)."""
    g = g12()
    for name in F1_CASE["scenes"]:
        assert len(calc.preds[name]) == int(g["ntrack_" + name]) and len(calc.gts[name]) == int(g["ngt_" + name])
        assert np.array_equal([t[0] for t in calc.preds[name]], g["trackcls_" + name])
        assert np.array_equal([t[-1] for t in calc.preds[name]], g["trackid_" + name])
        assert np.array_equal(np.array([t[2] for t in calc.preds[name]], np.float64), g["trackscore_" + name])
    assert set(metrics) == {"%s_%s" % (t, k) for t in (0.25, 0.5, 0.7) for k in ("accuracy", "recall", "f1")}
    for k, v in metrics.items():
        assert v == float(g["metric_" + k]), k


def duplicate_name_steps():
    """Two batches built from the g12 snippets in which scene_a appears twice (three times in the second), so that a later
    entry of a batch associates with tracks an earlier entry of the same batch created or changed."""
    st = f1_case_inputs(F1_CASE)
    a, b = st[0], st[2]                                            # both list scene_a, scene_b, scene_c
    first = dict(scenes=["scene_a", "scene_b", "scene_a"], corners=a["corners"], prob=a["prob"], mask=a["mask"], gts=a["gts"])
    second = dict(scenes=["scene_a", "scene_a", "scene_a"], corners=b["corners"], prob=b["prob"], mask=b["mask"], gts=b["gts"])
    return [first, second]


def run_steps(calc, steps, seed=99):
    np.random.seed(seed)
    for st in steps:
        _feed(calc, st)
    return calc


def tracker_state(calc):
    """Everything the stores hold, comparable with ==."""
    def flat(store):
        return {n: [(int(e[0]), np.asarray(e[1], np.float64).tolist(), float(e[2])) + ((int(e[3]),) if len(e) > 3 else ())
                    for e in trks] for n, trks in store.items()}
    return flat(calc.preds), flat(calc.gts)


def random_boxes(n, seed):
    """(n, 8, 3) canonical corners: boxes with sizes 0.25-1.5 and centres within a 3 m room, every third one tilted by up to 3
    degrees about both horizontal axes on top of its yaw."""
    rng = np.random.RandomState(seed)
    out = []
    for k in range(n):
        cen = rng.uniform(-1.5, 1.5, 3) * np.array([1, 1, 0.3])
        w = _yaw_box_corners(np.zeros(3), rng.uniform(0.125, 0.75, 3), rng.uniform(-np.pi, np.pi))
        if k % 3 == 2:
            ax, ay = np.deg2rad(rng.uniform(-3, 3, 2))
            Rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
            Ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
            w = w @ (Rx @ Ry).T
        out.append(canonical(w + cen))
    return np.stack(out)


class Recording:
    """Wraps an IoU backend and keeps every (segments, matrices) it served."""

    def __init__(self, inner):
        self.inner = inner
        self.calls = []

    def __call__(self, segments):
        mats = self.inner(segments)
        self.calls.append((segments, mats))
        return mats


def host_calculator():
    return F1Calculator(F1_CASE["conf"])

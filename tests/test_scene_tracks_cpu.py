"""CPU tier of the device tracker (parq_amd/scene_tracks.py, include/parq_hip.h parq_assign_max / parq_tracks_update): the NumPy
statements of tests/scene_tracks_cases.py against scipy, brute force and the unmodified host tracker, the generators' promise of
decision-safe inputs, the entry points' declaration and binding, and the argument checks that return before any device call."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest
import torch
from scipy.optimize import linear_sum_assignment

import parq_amd
from parq_amd import _lib
from parq_amd.f1_eval import F1Calculator
from parq_amd.scene_tracks import SceneTracks, check_tracks_args

import scene_tracks_cases as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("parq_assign_max_workspace_bytes", "parq_assign_max", "parq_tracks_store_bytes", "parq_tracks_update_workspace_bytes",
       "parq_tracks_update")


def scipy_r2c(m):
    rows, cols = linear_sum_assignment(-np.asarray(m, np.float64))
    out = -np.ones(m.shape[0], np.int32)
    out[rows] = cols
    return out


@pytest.mark.parametrize("k", range(len(T.DENSE_SHAPES)))
def test_assignment_statement_equals_scipy_on_dense_matrices(k):
    """Dense uniform float32 matrices have a unique optimum: the assignment must be identical."""
    m = T.dense_matrix(T.DENSE_SHAPES[k], 100 + k)
    r2c, u, v = T.assign_statement(m, with_duals=True)
    T.check_assignment_shape(r2c, *m.shape)
    assert np.array_equal(r2c, scipy_r2c(m))
    # the duals certify it: u_r + v_c <= -m[r][c] up to rounding, equal on the assigned pairs
    slack = -m.astype(np.float64) - u[:, None] - v[None, :]
    assert slack.min() > -1e-12
    assert max(abs(slack[r, c]) for r, c in enumerate(r2c.tolist()) if c >= 0) < 1e-12


def test_assignment_statement_on_iou_like_matrices():
    """Mostly zeros: ties decide among optimal assignments, so the comparison with scipy is the set of positive pairs."""
    cases = T.iou_like_cases()
    assert len(cases) == 65
    for k, m in enumerate(cases):
        r2c = T.assign_statement(m)
        T.check_assignment_shape(r2c, *m.shape)
        assert T.positive_pairs(m, r2c) == T.positive_pairs(m, scipy_r2c(m)), (k, m.shape)


def test_assignment_statement_on_the_hard_instance():
    assert np.array_equal(T.assign_statement(T.hard_matrix(64)), np.arange(64))
    assert np.array_equal(scipy_r2c(T.hard_matrix(64)), np.arange(64))


def test_assignment_statement_against_brute_force_up_to_6x6():
    cases = T.small_cases()
    assert sorted({m.shape for m in cases}) == sorted(itertools.product(range(1, 7), repeat=2)) and len(cases) == 72
    for m in cases:
        r2c = T.assign_statement(m)
        T.check_assignment_shape(r2c, *m.shape)
        assert abs(T.total(m, r2c) - T.brute_force_best(m)) < 1e-12, m.shape
    for shape in ((0, 4), (4, 0), (0, 0)):
        assert np.array_equal(T.assign_statement(np.zeros(shape, np.float32)), -np.ones(shape[0], np.int32))


def test_tie_rule_prefers_an_unassigned_column_then_the_lower_index():
    assert T.assign_statement(np.zeros((3, 5), np.float32)).tolist() == [0, 1, 2]
    assert T.assign_statement(np.zeros((5, 3), np.float32)).tolist() == [0, 1, 2, -1, -1]
    m = np.zeros((2, 3), np.float32)
    m[0, 1] = m[1, 1] = 0.5                      # both rows want column 1: row 0 keeps it, row 1 ends at the first free column
    assert T.assign_statement(m).tolist() == [1, 0]


def test_generators_are_decision_safe():
    T.assert_decision_safe(T.g12_steps(), T.F1_CASE["conf"])
    steps, _, _ = T.tracker_case()
    T.assert_decision_safe(steps, T.TRACKER_CASE["conf"])


def test_tracker_statement_equals_the_host_tracker_on_seeded_runs():
    steps, _, stores = T.tracker_case()
    calc = T.host_run(steps, T.TRACKER_CASE["conf"])
    assert set(stores) == set(calc.preds)
    for name, store in stores.items():
        assert T.store_tracks(store) == T.entry_tracks(calc.preds[name]), name
    over = T.overflow_step()
    stores, trace = T.run_statement([over], 8, 0.1)
    ids = trace[0]["track_id"][0]
    assert stores["full"]["count"] == 8 and stores["full"]["dropped"] == 4
    assert sorted(ids[ids != -1].tolist()) == [-2] * 4 + list(range(8))


def test_tracker_statement_on_the_g12_run_gives_the_reference_metrics():
    steps = T.g12_steps()
    stores, _ = T.run_statement(steps, 2048, T.F1_CASE["conf"])
    host = T.host_run(steps, T.F1_CASE["conf"], seed=T.F1_CASE["np_seed"])
    order_differs = 0
    for name, store in stores.items():
        assert T.store_tracks(store) == T.entry_tracks(host.preds[name]), name
        order_differs += [int(x) for x in store["labels"][:store["count"]]] != [t[0] for t in host.preds[name]]
    print("scenes whose tracks are numbered in another order than the host's: %d of %d" % (order_differs, len(stores)))
    # the statement's tracks in the host calculator's place: the nine metrics of the golden, exactly
    host.preds = {n: [[int(s["labels"][t]), s["corners"][t], s["scores"][t], t] for t in range(s["count"])] for n, s in stores.items()}
    g = T.g12_golden()
    metrics = host.compute_metrics()
    assert len(metrics) == 9
    for k, v in metrics.items():
        assert v == float(g["metric_" + k]), k


def test_header_declares_the_entry_points_and_the_binding_types_them():
    hdr = open(os.path.join(ROOT, "include", "parq_hip.h")).read()
    want = {"parq_assign_max": ["m", "m_total", "segments", "S", "max_rows", "max_cols", "workspace", "workspace_bytes", "row_to_col",
                                "out_total", "stream"],
            "parq_tracks_update": ["store", "S_cap", "max_tracks", "slots_host", "B", "corners_world", "sem_cls_prob", "pred_mask", "Q",
                                   "K", "conf_thresh", "iou_thresh", "workspace", "workspace_bytes", "track_id", "iou_out", "stream"],
            "parq_assign_max_workspace_bytes": ["S", "max_rows", "max_cols"], "parq_tracks_store_bytes": ["S_cap", "max_tracks"],
            "parq_tracks_update_workspace_bytes": ["B", "Q", "max_tracks"]}
    for name, names in want.items():
        m = re.search(r"\b(?:int|size_t)\s+\(%s\)\s*\(([^;]*)\)\s*;" % name, hdr)
        assert m, "include/parq_hip.h must declare %s" % name
        params = [p.strip() for p in re.sub(r"/\*.*?\*/", "", m.group(1).replace("\n", " ")).split(",")]
        assert [p.split()[-1].lstrip("*") for p in params] == names, name
        assert name in _lib.EXTRA_SYMBOLS and name not in _lib.SYMBOLS
        res, args = _lib.EXTRA_SYMBOLS[name]
        assert len(args) == len(names) and res is (C.c_size_t if name.endswith("bytes") else C.c_int)
    assert len(_lib.SYMBOLS) == 71 and len(_lib.SYMBOLS) + len(_lib.EXTRA_SYMBOLS) == 88      # 83 with these five; five added since
    assert "83" in open(os.path.join(ROOT, "README.md")).read() and "88" in open(os.path.join(ROOT, "README.md")).read()
    assert parq_amd.SceneTracks is SceneTracks


def test_library_exports_the_entry_points_and_sizes():
    lib = _lib.load()
    for name in NEW:
        fn = getattr(lib, name)
        assert fn.argtypes == _lib.EXTRA_SYMBOLS[name][1] and fn.restype is _lib.EXTRA_SYMBOLS[name][0]
    assert lib.parq_assign_max_workspace_bytes(3, 5, 7) == 3 * 12 * 8 and lib.parq_assign_max_workspace_bytes(1, 1, 0) == 16
    assert lib.parq_assign_max_workspace_bytes(1, 2049, 1) == 0 and lib.parq_assign_max_workspace_bytes(-1, 1, 1) == 0
    assert lib.parq_tracks_store_bytes(3, 96) == 3 * (2 + 26 * 96) * 4
    assert lib.parq_tracks_store_bytes(1, 2049) == 0 and lib.parq_tracks_store_bytes(1, 0) == 0
    per_scene = lib.parq_tracks_update_workspace_bytes(1, 70, 96)
    assert per_scene >= (3 * 70 + 70 * 96 + 2) * 4 and per_scene % 16 == 0
    assert lib.parq_tracks_update_workspace_bytes(5, 70, 96) == 5 * per_scene
    assert lib.parq_tracks_update_workspace_bytes(1, 2049, 8) == 0 and lib.parq_tracks_update_workspace_bytes(1, 8, 2049) == 0


def test_argument_errors_return_before_any_device_call():
    """PARQ_ERR_ARG (1) from checks made on the host: the pointers below are never dereferenced."""
    lib = _lib.load()
    p = C.c_void_p(4096)                                   # non-NULL, 16-byte aligned, never touched
    odd = C.c_void_p(4104)
    a = lambda *x: lib.parq_assign_max(*x)
    assert a(None, 0, None, 0, 4, 4, None, 0, None, 0, None) == 0            # S = 0: valid, nothing launched
    assert a(p, 16, p, -1, 4, 4, p, 64, p, 4, None) == 1
    assert a(p, -1, p, 1, 4, 4, p, 64, p, 4, None) == 1
    assert a(p, 16, p, 1, 2049, 4, p, 1 << 20, p, 4, None) == 1
    assert a(p, 16, p, 1, 4, 2049, p, 1 << 20, p, 4, None) == 1
    assert a(p, 16, p, 1, -1, 4, p, 64, p, 4, None) == 1
    assert a(None, 16, p, 1, 4, 4, p, 64, p, 4, None) == 1
    assert a(p, 16, None, 1, 4, 4, p, 64, p, 4, None) == 1
    assert a(p, 16, p, 1, 4, 4, p, 64, None, 4, None) == 1
    assert a(p, 16, p, 1, 4, 4, None, 64, p, 4, None) == 1
    assert a(p, 16, p, 1, 4, 4, p, 63, p, 4, None) == 1                      # 1 * (4 + 4) * 8 = 64 bytes needed
    assert a(p, 16, p, 1, 4, 4, odd, 64, p, 4, None) == 1
    assert b"parq_assign_max" in lib.parq_last_error()
    slots = (C.c_int32 * 2)(0, 1)
    need = lib.parq_tracks_update_workspace_bytes(2, 8, 8)

    def u(store=p, S_cap=2, mt=8, sl=slots, B=2, c=p, pr=p, mk=p, Q=8, K=10, ws=p, wsb=need, tid=p):
        return lib.parq_tracks_update(store, S_cap, mt, sl, B, c, pr, mk, Q, K, 0.1, 0.1, ws, wsb, tid, None, None)
    assert u(B=0) == 0                                                        # no scene: valid, nothing launched
    for bad in (dict(Q=0), dict(Q=2049), dict(mt=0), dict(mt=2049), dict(K=1), dict(B=-1), dict(S_cap=-1), dict(store=None),
                dict(sl=None), dict(c=None), dict(pr=None), dict(mk=None), dict(ws=None), dict(tid=None), dict(wsb=need - 1),
                dict(ws=odd), dict(S_cap=1), dict(sl=(C.c_int32 * 2)(1, 1)), dict(sl=(C.c_int32 * 2)(0, -1))):
        assert u(**bad) == 1, bad
    assert b"parq_tracks_update" in lib.parq_last_error()


def test_python_surface_checks_its_arguments_before_the_gpu():
    ok = dict(corners_world=torch.zeros(2, 5, 8, 3), sem_cls_prob=torch.zeros(2, 5, 10), pred_mask=torch.zeros(2, 5, dtype=torch.bool),
              n_names=2, num_classes=10)
    assert check_tracks_args(**ok) == (2, 5)
    for key, bad, match in (("corners_world", torch.zeros(2, 5, 8, 2), "corners_world must be"),
                            ("corners_world", torch.zeros(2, 5, 8, 3, dtype=torch.int32), "floating-point"),
                            ("sem_cls_prob", torch.zeros(2, 5, 9), "sem_cls_prob must be"), ("pred_mask", torch.zeros(2, 5), "pred_mask must be"),
                            ("pred_mask", torch.zeros(2, 4, dtype=torch.bool), "pred_mask must be"), ("n_names", 3, "scene names"),
                            ("corners_world", torch.zeros(2, 2049, 8, 3), "corners_world|sem_cls_prob")):
        a = dict(ok)
        a[key] = bad
        with pytest.raises(ValueError, match=match):
            check_tracks_args(**a)
    with pytest.raises(ValueError, match="Q = 2049"):
        check_tracks_args(torch.zeros(1, 2049, 8, 3), torch.zeros(1, 2049, 10), torch.zeros(1, 2049, dtype=torch.bool), 1, 10)
    for kw in (dict(max_tracks=0), dict(max_tracks=2049), dict(max_tracks=True), dict(num_classes=1)):
        with pytest.raises(ValueError):
            SceneTracks(**kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        SceneTracks(device="cpu")
    with pytest.raises(ValueError, match="track_store"):
        F1Calculator(0.1, track_store="gpu")
    with pytest.raises(ValueError, match="iou_device"):
        F1Calculator(0.1, track_store="device")
    assert F1Calculator(0.1).track_store == "host"
    from parq_amd.decoder import PARQDecoder
    assert PARQDecoder.tracks_on_device is False and callable(PARQDecoder.track)

"""GPU tier of the device tracker: parq_assign_max and parq_tracks_update (csrc/tracks.hip) against their NumPy statements
(tests/scene_tracks_cases.py) exactly, then SceneTracks through the evaluator and through PARQDecoder.track, and the promise that an
update neither copies to the host nor synchronises."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import eval_iou_cases as E
import scene_tracks_cases as T
from gpu_util import lib
from oracle.make_golden import F1_CASE
from parq_amd import Pose, SceneTracks, _lib, synth
from parq_amd.f1_eval import F1Calculator

pytestmark = pytest.mark.gpu

CANARY = -77


def vp(t):
    return C.c_void_p(t.data_ptr())


def pack(mats, max_rows, max_cols, canary_rows=3):
    """(m, table, out, offsets of each segment's output): the matrices back to back, canaries between the outputs."""
    table, flat, outs = [], [], []
    m_off, o_off = 0, canary_rows
    for m in mats:
        table.append((m_off, m.shape[0], m.shape[1], o_off))
        flat.append(m.reshape(-1))
        outs.append(o_off)
        m_off += m.size
        o_off += m.shape[0] + canary_rows
    m_all = torch.from_numpy(np.concatenate(flat)).cuda()
    return m_all, torch.tensor(table, dtype=torch.int64, device="cuda"), torch.full((o_off,), CANARY, dtype=torch.int32, device="cuda"), outs


def run_assign(m_all, table, out, max_rows, max_cols):
    l = lib()
    S = table.shape[0]
    need = l.parq_assign_max_workspace_bytes(S, max_rows, max_cols)
    ws = torch.zeros(max(need, 16), dtype=torch.uint8, device="cuda")
    rc = l.parq_assign_max(vp(m_all), m_all.numel(), vp(table), S, max_rows, max_cols, vp(ws), need, vp(out), out.numel(), _lib.stream_ptr())
    assert rc == 0, l.parq_last_error()
    return ws[:need].view(torch.float64).view(S, max_rows + max_cols)


def test_assign_max_one_launch_equals_the_statement():
    mats = T.launch_matrices()
    assert any(m.shape[0] == 0 for m in mats) and any(m.shape[1] == 0 for m in mats) and len(mats) > 140
    max_rows, max_cols = max(m.shape[0] for m in mats), max(m.shape[1] for m in mats)
    assert max_rows <= 512 and max_cols <= 512
    m_all, table, out, offs = pack(mats, max_rows, max_cols)
    duals = run_assign(m_all, table, out, max_rows, max_cols).cpu().numpy()
    got = out.cpu().numpy()
    covered = np.zeros(len(got), bool)
    for s, (m, o) in enumerate(zip(mats, offs)):
        want, u, v = T.assign_statement(m, with_duals=True)
        assert np.array_equal(got[o:o + m.shape[0]], want), (s, m.shape)
        assert np.array_equal(duals[s, :m.shape[0]], u) and np.array_equal(duals[s, max_rows:max_rows + m.shape[1]], v), (s, m.shape)
        covered[o:o + m.shape[0]] = True
    assert (got[~covered] == CANARY).all() and (~covered).sum() == 3 * (len(mats) + 1)
    # deterministic: the same bits from a second call; and from the large-LDS instantiation (bounds above 512)
    out2 = torch.full_like(out, CANARY)
    duals2 = run_assign(m_all, table, out2, max_rows, max_cols)
    assert torch.equal(out2, out) and np.array_equal(duals2.cpu().numpy().view(np.int64), duals.view(np.int64))
    out3 = torch.full_like(out, CANARY)
    run_assign(m_all, table, out3, 2048, 600)
    assert torch.equal(out3, out)


def test_assign_max_bad_table_rows_write_nothing():
    m = T.dense_matrix((5, 6), 3)
    m_all = torch.from_numpy(m.reshape(-1)).cuda()
    out = torch.full((16,), CANARY, dtype=torch.int32, device="cuda")
    rows = [(0, 5, 7, 0),            # 35 elements of 30
            (1, 5, 6, 0),            # starts one element late
            (0, 5, 6, 12),           # output rows 12..16 of 16
            (0, 9, 3, 0),            # more rows than max_rows
            (0, 3, 9, 0),            # more columns than max_cols
            (-1, 5, 6, 0), (0, -5, 6, 0), (0, 5, -6, 0), (0, 5, 6, -1), (1 << 40, 1 << 20, 1 << 20, 0)]
    table = torch.tensor(rows, dtype=torch.int64, device="cuda")
    run_assign(m_all, table, out, 8, 8)
    torch.cuda.synchronize()
    assert bool((out == CANARY).all())
    good = torch.tensor([(0, 5, 6, 11)], dtype=torch.int64, device="cuda")           # the last row that fits
    run_assign(m_all, good, out, 8, 8)
    got = out.cpu().numpy()
    assert np.array_equal(got[11:], T.assign_statement(m)) and (got[:11] == CANARY).all()


def raw_update(store, S_cap, mt, slots, st, conf, iou, want_iou=True):
    l = lib()
    B, Q = st["corners"].shape[:2]
    K = st["prob"].shape[2]
    corners, prob = torch.from_numpy(st["corners"]).cuda(), torch.from_numpy(st["prob"]).cuda()
    mask = torch.from_numpy(st["mask"].astype(np.uint8)).cuda()
    need = l.parq_tracks_update_workspace_bytes(B, Q, mt)
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    tid = torch.full((B, Q), CANARY, dtype=torch.int32, device="cuda")
    iou_out = torch.full((B, Q, mt), -1.0, dtype=torch.float32, device="cuda") if want_iou else None
    rc = l.parq_tracks_update(vp(store), S_cap, mt, (C.c_int32 * B)(*slots), B, vp(corners), vp(prob), vp(mask), Q, K, conf, iou, vp(ws), need,
                              vp(tid), vp(iou_out) if want_iou else None, _lib.stream_ptr())
    assert rc == 0, l.parq_last_error()
    return tid.cpu().numpy(), (iou_out.cpu().numpy() if want_iou else None)


def split_store(row, mt):
    return dict(count=int(row[0]), dropped=int(row[1]), labels=row[2:2 + mt], scores=row[2 + mt:2 + 2 * mt].view(np.float32),
                corners=row[2 + 2 * mt:].view(np.float32).reshape(mt, 8, 3))


def assert_store_equals(row, want, mt, what):
    got = split_store(row, mt)
    n = want["count"]
    assert (got["count"], got["dropped"]) == (n, want["dropped"]), what
    assert np.array_equal(got["labels"][:n], want["labels"][:n]), what
    assert np.array_equal(got["scores"][:n].view(np.int32), want["scores"][:n].view(np.int32)), what
    assert np.array_equal(got["corners"][:n].view(np.int32), want["corners"][:n].view(np.int32)), what
    assert not row[2 + n:2 + mt].any() and not got["scores"][n:].view(np.int32).any() and not got["corners"][n:].view(np.int32).any(), what


def test_tracks_update_equals_the_statement_after_every_step():
    c = T.TRACKER_CASE
    steps, trace, _ = T.tracker_case()
    mt, S_cap = c["max_tracks"], 5
    words = 2 + 26 * mt
    store = torch.zeros(S_cap, words, dtype=torch.int32, device="cuda")
    store[0] = CANARY
    store[4] = CANARY                                               # guard slots around the three in use: 3, 1, 2
    slots = [3, 1, 2]
    worst = 0.0
    for k, (st, tr) in enumerate(zip(steps, trace)):
        tid, iou = raw_update(store, S_cap, mt, slots, st, c["conf"], c["iou"])
        assert np.array_equal(tid, tr["track_id"]), k
        host = store.cpu().numpy()
        assert (host[0] == CANARY).all() and (host[4] == CANARY).all(), k
        for b, name in enumerate(st["scenes"]):
            assert_store_equals(host[slots[b]], tr["stores"][name], mt, (k, name))
            want = tr["ious"][b]
            D, n = want.shape
            got = iou[b, :D, :n]
            # float32(host iou3d) up to one float32 rounding of values the device IoU ties to the host's within 1e-12
            worst = max(worst, float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max()) if want.size else 0.0)
            assert np.array_equal(got == 0, want == 0), (k, name)
            assert (iou[b, D:] == -1.0).all() and (iou[b, :, n:] == -1.0).all(), (k, name)
    print("IoU output: max |device - float32(host)| = %.3e" % worst)
    assert worst <= 2.0 ** -23


def test_tracks_update_overflow_saturates_and_counts():
    st = T.overflow_step()
    stores, trace = T.run_statement([st], 8, 0.1)
    mt = 8
    store = torch.zeros(2, 2 + 26 * mt, dtype=torch.int32, device="cuda")
    store[1] = CANARY                                               # the guard rows behind the slot
    tid, _ = raw_update(store, 2, mt, [0], st, 0.1, 0.1, want_iou=False)
    assert np.array_equal(tid, trace[0]["track_id"])
    ids = tid[0][tid[0] != -1]
    assert ids.tolist() == list(range(8)) + [-2] * 4
    host = store.cpu().numpy()
    assert_store_equals(host[0], stores["full"], mt, "overflow")
    assert host[0, 0] == 8 and host[0, 1] == 4 and (host[1] == CANARY).all()
    # a corrupt count writes nothing: the slot stays as it is and nothing of its scene is a detection
    store[0, 0] = 9
    before = store.clone()
    tid, _ = raw_update(store, 2, mt, [0], st, 0.1, 0.1, want_iou=False)
    assert (tid == -1).all() and torch.equal(store, before)


def sorted_tracks(entries):
    return T.entry_tracks(entries)


def test_evaluator_with_the_device_track_store_on_the_g12_run():
    want = E.host_calculator()
    want_metrics = E.run_g12(want)
    calc = F1Calculator(F1_CASE["conf"], iou_device="cuda", track_store="device")
    metrics = E.run_g12(calc)
    g = E.g12()
    assert set(metrics) == set(want_metrics)
    for k, v in metrics.items():
        assert v == float(g["metric_" + k]) == want_metrics[k], k
    assert calc._tracks.enqueues == 4
    for name in F1_CASE["scenes"]:
        assert sorted_tracks(calc.preds[name]) == sorted_tracks(want.preds[name]), name
        assert [t[-1] for t in calc.preds[name]] == list(range(len(want.preds[name])))
        assert len(calc.gts[name]) == int(g["ngt_" + name])
    assert not any(calc._tracks.dropped().values())


def test_evaluator_duplicate_scene_names_with_the_device_track_store():
    steps = E.duplicate_name_steps()
    want = E.run_steps(E.host_calculator(), steps)
    calc = E.run_steps(F1Calculator(F1_CASE["conf"], iou_device="cuda", track_store="device"), steps)
    assert calc._tracks.enqueues == 2 + 3                                  # one enqueue per wave
    assert calc.compute_metrics() == want.compute_metrics()
    for name in want.preds:
        assert sorted_tracks(calc.preds[name]) == sorted_tracks(want.preds[name]), name
    assert E.tracker_state(calc)[1] == E.tracker_state(want)[1]           # the ground-truth store is the host's


def _tiny_decoder():
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "oracle"))
    from make_golden import PARSE_CASE, parse_case_inputs
    from parq_amd.decoder import PARQDecoder
    x = parse_case_inputs(PARSE_CASE)
    B, Q = PARSE_CASE["B"], PARSE_CASE["Q"]
    cfg = synth.decoder_cfg(dim=64, queries=Q, heads=1, ffn=64, layers=1)
    cfg.TRACK_SCALE = PARSE_CASE["track_scale"]
    dec = PARQDecoder(cfg).cuda().eval()
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    outs = [{"center_unnormalized": to(x["center"]), "size_unnormalized": to(x["size"]), "ortho6d": to(x["rot6"]),
             "sem_cls_prob": to(x["prob"])}]
    gt, _ = synth.make_boxes(77, B, 6, max_box=10)
    _, _, _, T_wl = synth.make_geometry(78, B, 2, 8, 10)
    return dec, outs, to(gt), to(T_wl), ["room0", "room1"]


def _upright_outputs():
    """A tiny decoder and outputs it could have produced: per scene five well separated upright boxes (object y along world z, the
    convention the tracker's IoU assumes) on odd queries below 20, background elsewhere.  The IoU routine's inside test is strict,
    so what a box's IoU with an exact copy of itself comes to is a question of rounding in the clip (the reference's routine, and the
    host's, behave the same).  The tests below are about ids, not about that: a probe run builds the world corners, and only the
    candidates whose host IoU with themselves is above 0.5 stay detections; the set-up asserts that at least three per scene do."""
    from parq_amd.decoder import PARQDecoder
    B, Q = 2, 32
    cfg = synth.decoder_cfg(dim=64, queries=Q, heads=1, ffn=64, layers=1)
    cfg.TRACK_SCALE = [-100.0, 100.0] * 3
    dec = PARQDecoder(cfg).cuda().eval()
    K = dec.num_semcls + 1
    rng = np.random.RandomState(3)
    center = rng.uniform(-40, 40, (B, Q, 3)).astype(np.float32)
    size = rng.uniform(0.4, 1.2, (B, Q, 3)).astype(np.float32)
    rot6 = np.zeros((B, Q, 6), np.float32)
    prob = np.full((B, Q, K), 0.01, np.float32)
    prob[..., K - 1] = 1.0 - 0.01 * (K - 1)
    for b in range(B):
        for q in range(Q):
            yaw = 0.2 * q + b
            rot6[b, q] = (np.cos(yaw), np.sin(yaw), 0.0, 0.0, 0.0, 1.0)
            if q < 20 and q % 2 == 1:
                center[b, q] = (2.0 * q, 3.0 * b, 0.5)
                prob[b, q] = 0.01
                prob[b, q, (q + b) % (K - 1)] = 1.0 - 0.01 * (K - 1) - 0.001 * q
    to = lambda a: torch.from_numpy(a).cuda()
    outs = [{"center_unnormalized": to(center), "size_unnormalized": to(size), "ortho6d": to(rot6), "sem_cls_prob": to(prob)}]
    T_wl = torch.tensor([1.0, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]).repeat(B, 1, 1).cuda()
    names = ["room0", "room1"]
    probe = dec.track([dict(outs[0])], Pose(T_wl), names, SceneTracks(max_tracks=64, num_classes=K))
    corners = probe["pred_corners_world"].cpu().numpy()
    for b in range(B):
        for q in range(1, 20, 2):
            if T.box_iou(corners[b, q], corners[b, q]) < 0.5:
                prob[b, q] = prob[b, 0]                              # background
        assert (prob[b].argmax(-1) != K - 1).sum() >= 3
    outs[0]["sem_cls_prob"] = to(prob)
    return dec, outs, T_wl, names


def test_decoder_tracks_on_device_gives_the_same_metrics():
    """The scenario of test_gpu_eval_iou.test_decoder_metrics_on_device: the same outputs fed twice."""
    from parq_amd import Obb3D
    from parq_amd.decoder import PARQDecoder
    assert PARQDecoder.tracks_on_device is False
    dec, outs, gt, T_wl, names = _tiny_decoder()
    dec.metrics_on_device = True
    results = {}
    for on in (False, True):
        dec.tracks_on_device = on
        np.random.seed(11)
        dec.reset_metrics()
        calc = dec.metrics_calculator[0]
        for _ in range(2):
            dec.update_metrics(outs, Obb3D(gt), Pose(T_wl), names)
        assert calc.on_device_tracks == on
        metrics = dec.compute_metrics()
        results[on] = (metrics, {n: sorted_tracks(t) for n, t in calc.preds.items()}, E.tracker_state(calc)[1])
    assert results[True] == results[False]
    assert min(len(t) for t in results[True][1].values()) > 3


def test_decoder_track_gives_stable_ids_and_counts():
    dec, outs, T_wl, names = _upright_outputs()
    tracks = SceneTracks(max_tracks=64, num_classes=dec.num_semcls + 1)
    first = dec.track(outs, Pose(T_wl), names, tracks)["track_id"].clone()
    out = dec.track(outs, Pose(T_wl), names, tracks)
    second = out["track_id"]
    assert second.dtype == torch.int32 and second.shape == out["pred_mask"].shape and second.is_cuda
    kept = [T.select(out["sem_cls_prob"][b].cpu().numpy(), out["pred_mask"][b].cpu().numpy(), tracks.conf_thresh)[0]
            for b in range(len(names))]
    for b, name in enumerate(names):
        ids1, ids2 = first[b].cpu().numpy(), second[b].cpu().numpy()
        det = np.zeros(len(ids1), bool)
        det[kept[b]] = True
        assert (ids1[~det] == -1).all() and (ids2[~det] == -1).all()
        assert np.array_equal(ids1[det], np.arange(det.sum()))              # a first visit numbers the detections in query order
        assert np.array_equal(ids2, ids1), name                             # every detection meets itself again
        view = tracks.boxes(name)
        assert view["count"].ndim == 0 and view["count"].dtype == torch.int32 and int(view["count"]) == det.sum() >= 3
        assert view["corners"].shape == (64, 8, 3) and view["corners"].data_ptr() == tracks._store[tracks._slots[name]][2 + 128:].data_ptr()
        assert torch.equal(view["corners"][:det.sum()], out["pred_corners_world"][b][torch.from_numpy(det).cuda()])
        host = tracks.to_host(name)
        assert [e[3] for e in host] == list(range(det.sum())) and [e[0] for e in host] == view["labels"][:det.sum()].tolist()
    assert tracks.dropped() == {"room0": 0, "room1": 0}
    tracks.reset("room0")
    assert int(tracks.boxes("room0")["count"]) == 0 and int(tracks.boxes("room1")["count"]) >= 3
    tracks.reset()
    assert tracks.names() == [] and tracks.to_host() == {}


def test_store_grows_without_losing_tracks():
    st = T.overflow_step()
    tracks = SceneTracks(max_tracks=16)
    dev = lambda a: torch.from_numpy(a).cuda()
    first = tracks.update(["scene0"], dev(st["corners"]), dev(st["prob"]), dev(st["mask"]))
    for k in range(1, 12):                                                   # past the first allocation of 8 slots
        tracks.update(["scene%d" % k], dev(st["corners"]), dev(st["prob"]), dev(st["mask"]))
    again = tracks.update(["scene0"], dev(st["corners"]), dev(st["prob"]), dev(st["mask"]))
    stores, trace = T.run_statement([st, st], 16, 0.1)                      # what scene0 saw: the same step twice
    assert np.array_equal(first.cpu().numpy(), trace[0]["track_id"]) and np.array_equal(again.cpu().numpy(), trace[1]["track_id"])
    assert (trace[1]["track_id"] >= 0).sum() == 12 and (trace[1]["track_id"][trace[0]["track_id"] >= 0] < 12).sum() >= 6
    assert int(tracks.boxes("scene0")["count"]) == stores["full"]["count"] and int(tracks.boxes("scene11")["count"]) == 12


def test_update_and_track_do_not_synchronise():
    dec, outs, T_wl, names = _upright_outputs()
    tracks = SceneTracks(max_tracks=64, num_classes=dec.num_semcls + 1)
    pose = Pose(T_wl)
    out = dec.track(outs, pose, names, tracks)                               # warm-up: allocations, library load
    corners, prob, mask = out["pred_corners_world"].clone(), out["sem_cls_prob"].clone(), out["pred_mask"].clone()
    tracks.update(names, corners, prob, mask)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        ids = tracks.update(names, corners, prob, mask)
        out = dec.track(outs, pose, names, tracks)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(ids, out["track_id"]) and int((ids >= 0).sum()) >= 6

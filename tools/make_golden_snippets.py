"""Write tests/golden/g25_snippets.npz: the reference's own snippet annotation on the cases of tests/snippet_cases.py.

Development container only (it imports the reference tree through oracle.reference_loader; run from the repository root:
``python tools/make_golden_snippets.py``).  The reference's script directory is put on the path, an empty ``quaternion`` module
into ``sys.modules`` (``cv2`` is stubbed by the loader; its ``imread`` hands out the case's generated depth) and ``torch.Tensor.cuda``
is the identity for the length of the run.  Per case and scene the reference's own ``get_point_cloud``,
``get_point_cloud_inside_box3d``, ``get_box3d_inside_fov`` and ``get_level`` run on every frame, the snippet maxima and the
valid-object filter follow generate_scannet_anno_snippet.py:243-246,317-329, and the kept boxes go through ``ToTensor`` +
``Convert2Objects``.  The four ``view_selection*`` functions run on the trajectory of ``snippet_cases.make_trajectory``.  Stored are
results only: counts, ratios, levels, valid lists, ``obbs_padded`` / ``sym`` / ``num_valid`` and the selected id lists.

So that equality with the reference does not rest on a summation order, the tool asserts that no fixture point lies within a
relative 1e-9 of a box face, that no snippet-level count equals a threshold and that no ratio lies within 1e-4 of a ratio threshold.
It also writes profiles/snippet_targets_parity.txt: the largest difference between the statement's and the reference's ratios.
"""
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import snippet_cases as SC  # noqa: E402
from oracle import reference_loader  # noqa: E402

PARITY = os.path.join(ROOT, "profiles", "snippet_targets_parity.txt")
SELECT = [dict(window_size=3, min_angle=15.0, min_distance=0.1), dict(window_size=1, min_angle=15.0, min_distance=0.1),
          dict(window_size=2, min_angle=8.0, min_distance=0.05)]


def load_reference():
    reference_loader.load()
    sys.path.insert(0, os.path.join(reference_loader.REFERENCE_ROOT, "scripts", "scannet_preprocessing"))
    sys.modules.setdefault("quaternion", types.ModuleType("quaternion"))
    import processing_utils as PU
    from datasets import transforms as RT
    return PU, RT


def face_margin(points, cam):
    """The smallest |m_e| / vv_e and |m_e - vv_e| / vv_e over all points, boxes and edges (float64)."""
    o, e, vv = SC.box_edges(cam)
    pts = points.astype(np.float64)
    worst = np.inf
    for n in range(len(cam)):
        m = (pts - o[n]) @ e[n].T
        worst = min(worst, float(np.minimum(np.abs(m), np.abs(m - vv[n])).__truediv__(vv[n]).min()) if len(pts) else np.inf)
    return worst


def run_scene(PU, RT, d, b, n_real, name):
    """One scene of a case through the reference's functions; arrays sized N (padding rows: count 0, ratio 0, level 3)."""
    depth, Kd, Kc = d["depth"][b], d["depth_intrinsics"][b], d["color_intrinsics"][b]
    (h, w), poses, rows = d["color_size"], d["T_world_camera"][b], d["obbs"][b]
    T, N = depth.shape[0], rows.shape[0]
    fp, ft = np.zeros((T, N), np.int32), np.zeros((T, N), np.float32)
    margin, statement_diff = np.inf, 0.0
    if n_real:
        cw = (SC.rows_corners_world(rows) if d["corners_world"] is None else d["corners_world"][b])[:n_real]
        bbox_corners = torch.from_numpy(np.ascontiguousarray(cw))
        counts, ratios = [], []
        for t in range(T):
            sys.modules["cv2"].imread = lambda path, flag, _t=t: depth[_t].copy()
            T_camera_scan = torch.from_numpy(np.linalg.inv(poses[t]))
            cam = (PU.get_homogeneous(bbox_corners.view(-1, 3)) @ T_camera_scan.T)[:, :3].view(-1, 8, 3)
            pc = PU.get_point_cloud("frame-%06d.depth.pgm" % t, Kd)
            inside, _ = PU.get_point_cloud_inside_box3d(cam, pc)
            ratio, _ = PU.get_box3d_inside_fov(cam, (h, w, 3), Kc)
            counts.append(inside)
            ratios.append(ratio)
            fp[t, :n_real], ft[t, :n_real] = inside.numpy(), ratio.numpy()
            margin = min(margin, face_margin(pc.numpy(), cam.numpy()))
            own = SC.truncation(SC.camera_corners(poses[t], cw), Kc, (h, w))
            statement_diff = max(statement_diff, SC.parity(own, ratio.numpy()))
        points = torch.stack(counts).max(dim=0)[0]
        trunc = torch.stack(ratios).max(dim=0)[0]
        levels = [PU.get_level(points[i], trunc[i]) for i in range(n_real)]
        valid_obj = [i for i in range(n_real) if not levels[i] >= 3]
        assert not np.isin(points.numpy(), [pc_ for pc_, _ in SC.DEFAULT_LEVELS]).any(), (name, b, "a count equals a threshold")
        for _, tr in SC.DEFAULT_LEVELS:
            assert np.abs(trunc.numpy().astype(np.float64) - tr).min() > 1e-4, (name, b, "a ratio within 1e-4 of %g" % tr)
    else:
        points, trunc, levels, valid_obj = torch.zeros(0, dtype=torch.int64), torch.zeros(0), [], []
    assert margin > 1e-9, (name, b, "a point within %.3e of a box face" % margin)
    S = d["sym"].shape[1]
    obbs_padded = -np.ones((100, 19), np.float32)
    sym = [d["sym"][b, i] if i < S else -1 for i in valid_obj]
    if valid_obj:
        T_so = np.tile(np.eye(4), (len(valid_obj), 1, 1))
        T_so[:, :3, :3] = rows[valid_obj, 6:15].reshape(-1, 3, 3)
        T_so[:, :3, 3] = rows[valid_obj, 15:18]
        data = {"rgb_img": [np.zeros((4, 4, 3), np.uint8)] * T, "intrinsics": np.stack([Kc[:3, :3]] * T), "T_world_camera": poses.copy(),
                "bboxes": rows[valid_obj, 0:6], "T_world_object": T_so, "label": [float(v) for v in rows[valid_obj, 18]], "sym": sym}
        out = RT.Convert2Objects(T)(RT.ToTensor()(data))
        obbs_padded = out["obbs_padded"]._data.numpy().astype(np.float32)
        assert obbs_padded.shape == (100, 19)
    sym_out = -np.ones(S, d["sym"].dtype)
    sym_out[:min(len(sym), S)] = sym[:S]
    full = lambda a, fill, dt: np.concatenate([np.asarray(a, dt), np.full(N - n_real, fill, dt)])
    return dict(frame_points=fp, frame_truncation=ft, points_inside=full(points.numpy(), 0, np.int32),
                truncation=full(trunc.numpy(), 0, np.float32), difficulty=full(levels, 3, np.int32),
                valid=np.isin(np.arange(N), valid_obj), obbs_padded=obbs_padded, sym=sym_out,
                num_valid=np.int32(len(valid_obj))), margin, statement_diff


def main():
    PU, RT = load_reference()
    cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    arrays, worst_margin, worst_diff, seen_levels = {}, np.inf, 0.0, set()
    try:
        for c in SC.CASES:
            d = SC.make_case(c)
            per = []
            for b in range(c["B"]):
                res, margin, diff = run_scene(PU, RT, d, b, c["n"][b], c["name"])
                per.append(res)
                worst_margin, worst_diff = min(worst_margin, margin), max(worst_diff, diff)
                seen_levels |= set(res["difficulty"][:c["n"][b]].tolist())
            for key in per[0]:
                arrays[c["name"] + "/" + key] = np.stack([r[key] for r in per])
            print("%s: counts %s ... valid %s" % (c["name"], arrays[c["name"] + "/points_inside"][0][:8].tolist(),
                                                 arrays[c["name"] + "/num_valid"].tolist()))
        lv = SC.case_by_name("levels_96x128")
        pts = arrays[lv["name"] + "/points_inside"]
        for thr, _ in SC.DEFAULT_LEVELS:
            assert (pts[pts > 0] < thr).any() and (pts > thr).any(), "counts on one side of %d only" % thr
        assert seen_levels == {0, 1, 2, 3}, seen_levels
        # frame selection: the dict the reference's loader leaves (frames with a non-finite pose are absent)
        traj = SC.make_trajectory()
        cam_pose_list = {i: M for i, M in enumerate(traj) if not (M[0][0] == np.inf or M[0][0] == -np.inf)}
        select = []
        for kw in SELECT:
            args = types.SimpleNamespace(**kw)
            select.append(dict(kw, val=PU.view_selection(args, "s", cam_pose_list), w1=PU.view_selection_w1(args, "s", cam_pose_list),
                               train=PU.view_selection_overlap(args, "s", cam_pose_list),
                               all=PU.view_selection_allframes(args, "s", cam_pose_list)))
            print("select %s: %d val, %d w1, %d train, %d key frames" % (kw, len(select[-1]["val"]), len(select[-1]["w1"]),
                                                                          len(select[-1]["train"]), len(select[-1]["all"][0])))
    finally:
        torch.Tensor.cuda = cuda
    meta = {"cases": SC.CASES, "select": json.loads(json.dumps(select, default=int))}
    arrays["meta"] = np.frombuffer(json.dumps(meta, sort_keys=True).encode(), dtype=np.uint8)
    np.savez_compressed(SC.GOLDEN, **arrays)
    print("wrote %s (%d arrays, %d bytes)" % (SC.GOLDEN, len(arrays), os.path.getsize(SC.GOLDEN)))
    with open(PARITY, "w") as f:
        f.write("python tools/make_golden_snippets.py\n"
                "truncation ratios, NumPy statement (tests/snippet_cases.py) against the reference's get_box3d_inside_fov, all cases:\n"
                "largest max |a - b| / max(1, |b|) = %.3e   (the tests' bound: 1e-4)\n"
                "counts, levels, valid lists, obbs_padded, sym: equal (asserted by tests/test_snippets_cpu.py)\n"
                "smallest relative distance of a fixture point to a box face: %.3e   (asserted above 1e-9)\n" % (worst_diff, worst_margin))
    print(open(PARITY).read())


if __name__ == "__main__":
    main()

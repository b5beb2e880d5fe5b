"""Cases, inputs and the NumPy statement of the snippet targets (parq_amd/snippets.py, include/parq_hip.h parq_snippet_targets).

The rule restates the reference's offline annotation pass (scripts/scannet_preprocessing/processing_utils.py:132-154,206-263,304-336
and generate_scannet_anno_snippet.py:189-256,317-329) with every summation order fixed: ``statement`` below is that rule in NumPy,
operation by operation as include/parq_hip.h writes it.  tests/golden/g25_snippets.npz holds what the reference's own functions gave
for every case (tools/make_golden_snippets.py: results only); the statement is pinned to those and the kernels to the statement, bit
for bit.  Inputs are generated from the case's seed — depth as slanted and stepped surfaces in integer millimetres with holes of
zeros, boxes placed on those surfaces — so that no depth is stored.
"""
import json
import os

import numpy as np

G25 = "g25_snippets"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", G25 + ".npz")
TILE_PIXELS = 2048                      # pixels of a counting workgroup (csrc/snippets.hip kTileWords * 4)
DEFAULT_LEVELS = ((1000, 0.85), (500, 0.70), (100, 0.50))
PICK = ((0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1))      # Obb3D.bb3corners_object

# depth = (H, W); color = (h, w); n = boxes per scene (N = max(n)); S = width of sym; special = what the case is there for
CASES = [
    dict(name="levels_96x128", seed=11, B=2, T=3, depth=(96, 128), color=(192, 256), n=(24, 17), S=30, special="levels"),
    dict(name="odd_61x77", seed=12, B=1, T=2, depth=(61, 77), color=(121, 155), n=(7,), S=7),            # odd rows, a frame tail, 3 tiles
    dict(name="n128_32x40", seed=13, B=1, T=2, depth=(32, 40), color=(64, 80), n=(128,), S=128, sym_int=True),
    dict(name="n1_and_padding", seed=14, B=2, T=2, depth=(32, 40), color=(64, 80), n=(1, 0), S=1),
    dict(name="zero_frame", seed=15, B=1, T=2, depth=(32, 40), color=(64, 80), n=(5,), S=5, zero_frames=(0,)),
    dict(name="clamp_t1", seed=16, B=1, T=1, depth=(61, 77), color=(121, 155), n=(6,), S=6, special="clamp"),
    dict(name="nothing_valid", seed=17, B=1, T=2, depth=(32, 40), color=(64, 80), n=(4,), S=4, special="far"),
    dict(name="six_digits", seed=18, B=1, T=3, depth=(61, 77), color=(121, 155), n=(9,), S=12, digits=6, corners=True),
]
# other thresholds than the reference's, on the same inputs: against the statement only
LEVEL_VARIANTS = [
    dict(case="n128_32x40", levels=((40, 0.5), (10, 0.3), (0, 0.05)), max_level=3, max_box=100),          # more than max_box valid rows
    dict(case="levels_96x128", levels=((700, 0.9), (50, 0.2)), max_level=1, max_box=5),
]


def case_by_name(name):
    return next(c for c in CASES if c["name"] == name)


def _rot(rng, small=False):
    """A rotation matrix (float64) from three seeded angles."""
    a, b, c = rng.uniform(-0.25, 0.25, 3) if small else rng.uniform(-np.pi, np.pi, 3)
    ca, sa, cb, sb, cc, sc = np.cos(a), np.sin(a), np.cos(b), np.sin(b), np.cos(c), np.sin(c)
    Rz = np.array([[ca, -sa, 0], [sa, ca, 0], [0, 0, 1.0]])
    Ry = np.array([[cb, 0, sb], [0, 1.0, 0], [-sb, 0, cb]])
    Rx = np.array([[1.0, 0, 0], [0, cc, -sc], [0, sc, cc]])
    return Rz @ Ry @ Rx


def _surface(rng, H, W, near):
    """(H, W) integer millimetres: a slanted plane with steps and holes of zeros."""
    y, x = np.mgrid[0:H, 0:W]
    z0 = rng.randint(600, 900) if near else rng.randint(1400, 2600)
    mm = z0 + (x * rng.randint(-3, 4)) // 2 + (y * rng.randint(-3, 4)) // 2
    mm = mm + 150 * ((x // max(8, W // 5) + y // max(8, H // 4)) % 2)                       # steps
    for _ in range(3):                                                                      # holes
        hy, hx = rng.randint(0, H), rng.randint(0, W)
        mm[hy:hy + rng.randint(2, max(3, H // 8)), hx:hx + rng.randint(2, max(3, W // 8))] = 0
    return np.clip(mm, 0, 65535).astype(np.uint16)


def _intrinsics(h, w, f):
    K = np.eye(4, dtype=np.float32)
    K[0, 0], K[1, 1], K[0, 2], K[1, 2] = f, f * 1.01, (w - 1) / 2 + 0.37, (h - 1) / 2 - 0.21
    return K


def make_case(c):
    """The inputs of a case, all NumPy: depth (B, T, H, W) uint16, depth_intrinsics / color_intrinsics (B, 4, 4) float32, color_size
    (h, w), T_world_camera (B, T, 4, 4) float64, obbs (B, N, 19) float32 with -1 padding, sym (B, S) float32 or int32,
    corners_world (B, N, 8, 3) float64 or None."""
    rng = np.random.RandomState(c["seed"])
    B, T, (H, W), (h, w) = c["B"], c["T"], c["depth"], c["color"]
    N = max(max(c["n"]), 1)
    near = c.get("special") == "clamp"
    Kd = np.stack([_intrinsics(H, W, 0.9 * W + b) for b in range(B)])
    Kc = np.stack([_intrinsics(h, w, 0.9 * w + 2 * b) for b in range(B)])
    depth = np.stack([np.stack([_surface(rng, H, W, near) for _ in range(T)]) for _ in range(B)])
    for t in c.get("zero_frames", ()):
        depth[:, t] = 0
    t_ref = min(t for t in range(T) if t not in c.get("zero_frames", ()))                   # the frame the boxes are placed on
    poses = np.zeros((B, T, 4, 4), np.float64)
    obbs = -np.ones((B, N, 19), np.float32)
    for b in range(B):
        R0, t0 = _rot(rng), rng.uniform(-2, 2, 3)
        for t in range(T):
            dR = _rot(rng, small=True) if t else np.eye(3)
            poses[b, t, :3, :3] = R0 @ dR
            poses[b, t, :3, 3] = t0 + (rng.uniform(-0.1, 0.1, 3) if t else 0)
            poses[b, t, 3, 3] = 1
        if "digits" in c:
            poses[b] = np.round(poses[b], c["digits"])
        fx, fy, cx, cy = (float(v) for v in (Kd[b, 0, 0], Kd[b, 1, 1], Kd[b, 0, 2], Kd[b, 1, 2]))
        for i in range(c["n"][b]):
            # a pixel of the placing frame's surface, the camera point behind it, a box around that point sized for a target pixel count
            u, v = rng.randint(W // 8, W - W // 8), rng.randint(H // 8, H - H // 8)
            D = max(int(depth[b, t_ref, v, u]), 500) / 1000.0
            target = (30, 70, 200, 400, 650, 900, 1300, 2200)[i % 8] * (H * W) / (96.0 * 128.0)
            side = np.sqrt(max(target, 4.0)) * D / fx
            size = side * rng.uniform(0.8, 1.25, 3)
            centre = np.array([(u - cx) / fx * D, (v - cy) / fy * D, D])
            Rco = _rot(rng)
            if c.get("special") == "clamp":
                if i == 0:                                   # encloses the camera
                    centre, size = np.array([0.05, -0.03, 0.1]), np.array([3.0, 2.5, 4.0])
                elif i == 1:                                 # nearer than 1 m: the max(z, 1) clamp
                    centre, size = np.array([0.02, 0.01, 0.45]), np.array([0.3, 0.25, 0.2])
                elif i == 2:                                 # wholly outside the image, to the right
                    centre, size = np.array([6.0, 0.1, 1.5]), np.array([0.4, 0.4, 0.4])
                elif i == 3:                                 # behind the camera
                    centre, size = np.array([0.1, 0.1, -1.5]), np.array([0.5, 0.5, 0.5])
            if c.get("special") == "far":                    # off the surfaces and small: nothing is visible enough
                centre = centre + np.array([0.0, 0.0, 1.5])
                size = size * 0.2
            if c.get("special") == "levels" and i % 6 == 5:  # partly outside the image: ratios below 1
                centre = centre + np.array([(W - 1 - cx) / fx * D - centre[0], 0.0, 0.0]) * rng.uniform(0.8, 1.1)
            Rwo = poses[b, t_ref, :3, :3] @ Rco
            two = poses[b, t_ref, :3, :3] @ centre + poses[b, t_ref, :3, 3]
            obbs[b, i, 0:6] = np.stack([-size / 2, size / 2], 1).reshape(6)
            obbs[b, i, 6:15] = Rwo.reshape(9)
            obbs[b, i, 15:18] = two
            obbs[b, i, 18] = rng.randint(0, 9)
    S = c["S"]
    sym = rng.randint(0, 4, (B, S))
    for b in range(B):
        sym[b, min(c["n"][b], S):] = -1
    sym = sym.astype(np.int32 if c.get("sym_int") else np.float32)
    corners = None
    if c.get("corners"):
        corners = rows_corners_world(obbs) + rng.uniform(-1e-9, 1e-9, (B, N, 8, 3))          # not representable in float32
    return dict(depth=depth, depth_intrinsics=Kd, color_intrinsics=Kc, color_size=(h, w), T_world_camera=poses, obbs=obbs, sym=sym,
                corners_world=corners)


# ---- the statement --------------------------------------------------------------------------------------------------------------
def rows_corners_world(obbs):
    """(..., 8, 3) float64: the corners of float32 rows in the world frame, w_i = ((R_i0 cx + R_i1 cy) + R_i2 cz) + t_i."""
    r = np.asarray(obbs, np.float32).astype(np.float64)
    out = np.zeros(r.shape[:-1] + (8, 3), np.float64)
    for k, (sx, sy, sz) in enumerate(PICK):
        cx, cy, cz = r[..., sx], r[..., 2 + sy], r[..., 4 + sz]
        for i in range(3):
            out[..., k, i] = ((r[..., 6 + 3 * i] * cx + r[..., 7 + 3 * i] * cy) + r[..., 8 + 3 * i] * cz) + r[..., 15 + i]
    return out


def affine_inverse(M):
    """(Ri (3, 3), ti (3,)) of a 4 x 4 float64 pose: the 3 x 3 block by cofactors, the bottom row taken as 0 0 0 1."""
    a = np.asarray(M, np.float64)
    a00, a01, a02, a10, a11, a12, a20, a21, a22 = (float(a[i, j]) for i in range(3) for j in range(3))
    c00, c01, c02 = a11 * a22 - a12 * a21, a10 * a22 - a12 * a20, a10 * a21 - a11 * a20
    with np.errstate(all="ignore"):
        det = np.float64((a00 * c00 - a01 * c01) + a02 * c02)
        Ri = np.array([[c00, a02 * a21 - a01 * a22, a01 * a12 - a02 * a11],
                       [a12 * a20 - a10 * a22, a00 * a22 - a02 * a20, a02 * a10 - a00 * a12],
                       [c02, a01 * a20 - a00 * a21, a00 * a11 - a01 * a10]], np.float64) / det
    t = a[:3, 3]
    ti = -((Ri[:, 0] * t[0] + Ri[:, 1] * t[1]) + Ri[:, 2] * t[2])
    return Ri, ti


def camera_corners(M, corners_world):
    """(N, 8, 3) float64: q_i = ((Ri_i0 w0 + Ri_i1 w1) + Ri_i2 w2) + ti_i."""
    Ri, ti = affine_inverse(M)
    w = corners_world
    return np.stack([((Ri[i, 0] * w[..., 0] + Ri[i, 1] * w[..., 1]) + Ri[i, 2] * w[..., 2]) + ti[i] for i in range(3)], -1)


def frame_points(depth, Ki, depth_scale=1000):
    """(P, 3) float32 points of the pixels with p_2 > 0, in pixel order, and the (H, W) mask of those pixels."""
    H, W = depth.shape
    Ki = np.asarray(Ki, np.float32)
    d = depth.astype(np.float32) / np.float32(depth_scale)
    y, x = np.mgrid[0:H, 0:W]
    v0, v1 = x.astype(np.float32) * d, y.astype(np.float32) * d
    p = [((Ki[i, 0] * v0 + Ki[i, 1] * v1) + Ki[i, 2] * d) + Ki[i, 3] for i in range(3)]
    assert all(q.dtype == np.float32 for q in p)
    keep = p[2] > 0
    return np.stack([q[keep] for q in p], -1), keep


def box_edges(cam):
    """origin (N, 3), edges (N, 3, 3) to corners 5, 0, 7 and their squared lengths (N, 3), float64."""
    o = cam[:, 4]
    e = np.stack([cam[:, 5] - o, cam[:, 0] - o, cam[:, 7] - o], 1)
    vv = (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]
    return o, e, vv


def points_inside(points, cam):
    """(N,) int32: points with 0 < m_e < vv_e for the three edges of every box."""
    o, e, vv = box_edges(cam)
    pts = points.astype(np.float64)
    out = np.zeros(len(cam), np.int32)
    for n in range(len(cam)):
        r = pts - o[n]
        ok = np.ones(len(pts), bool)
        for k in range(3):
            m = (r[:, 0] * e[n, k, 0] + r[:, 1] * e[n, k, 1]) + r[:, 2] * e[n, k, 2]
            ok &= (0 < m) & (m < vv[n, k])
        out[n] = ok.sum()
    return out


def truncation(cam, Kc, color_size):
    """(N,) float32: the share of every box's projected 2-D extent inside the (h, w) colour image."""
    h, w = color_size
    Kc = np.asarray(Kc, np.float32)
    c = cam.astype(np.float32)
    x, y, z = c[..., 0], c[..., 1], c[..., 2]
    P = [((Kc[i, 0] * x + Kc[i, 1] * y) + Kc[i, 2] * z) + Kc[i, 3] for i in range(3)]
    one, zero = np.float32(1), np.float32(0)
    zc = np.where(P[2] > one, P[2], one)
    u, v = P[0] / zc, P[1] / zc
    xmin, xmax, ymin, ymax = u[:, 0], u[:, 0], v[:, 0], v[:, 0]
    for k in range(1, 8):
        xmin, xmax = np.where(u[:, k] < xmin, u[:, k], xmin), np.where(u[:, k] > xmax, u[:, k], xmax)
        ymin, ymax = np.where(v[:, k] < ymin, v[:, k], ymin), np.where(v[:, k] > ymax, v[:, k], ymax)
    area = (xmax - xmin) * (ymax - ymin)
    clip = lambda a, hi: np.where(a < zero, zero, np.where(a > np.float32(hi), np.float32(hi), a))
    inside = (clip(xmax, w - 1) - clip(xmin, w - 1)) * (clip(ymax, h - 1) - clip(ymin, h - 1))
    ratio = inside / np.where(area > one, area, one)
    assert ratio.dtype == np.float32
    return ratio


def level_of(count, ratio, levels=DEFAULT_LEVELS):
    for i, (pc, tr) in enumerate(levels):
        if count > pc and np.float32(ratio) > np.float32(tr):
            return i
    return len(levels)


def statement(depth, depth_intrinsics_inv, color_intrinsics, color_size, T_world_camera, obbs, sym, corners_world=None,
              levels=DEFAULT_LEVELS, max_level=3, depth_scale=1000, max_box=100):
    """The whole rule.  Returns frame_points / frame_truncation (B, T, N), points_inside / truncation / difficulty / valid (B, N),
    obbs_padded (B, max_box, 19), sym (B, S), num_valid (B,)."""
    B, T = depth.shape[:2]
    N, S = obbs.shape[1], sym.shape[1]
    pad = np.all(obbs == -1, -1)
    cw = rows_corners_world(obbs) if corners_world is None else np.asarray(corners_world, np.float64)
    fp, ft = np.zeros((B, T, N), np.int32), np.zeros((B, T, N), np.float32)
    for b in range(B):
        for t in range(T):
            cam = camera_corners(T_world_camera[b, t], cw[b])
            pts, _ = frame_points(depth[b, t], depth_intrinsics_inv[b], depth_scale)
            fp[b, t] = np.where(pad[b], 0, points_inside(pts, cam))
            ft[b, t] = np.where(pad[b], np.float32(0), truncation(cam, color_intrinsics[b], color_size))
    points, trunc = fp.max(1), ft.max(1)
    diff = np.array([[level_of(points[b, n], trunc[b, n], levels) for n in range(N)] for b in range(B)], np.int32).reshape(B, N)
    valid = ~pad & (diff < max_level)
    out_rows = -np.ones((B, max_box, 19), np.float32)
    out_sym = -np.ones((B, S), sym.dtype)
    num = np.zeros(B, np.int32)
    for b in range(B):
        idx = np.nonzero(valid[b])[0]
        k = min(len(idx), max_box)
        out_rows[b, :k] = obbs[b, idx[:k]]
        for j, n in enumerate(idx[:S]):
            out_sym[b, j] = sym[b, n] if n < S else -1
        num[b] = k
    return dict(frame_points=fp, frame_truncation=ft, points_inside=points, truncation=trunc, difficulty=diff, valid=valid,
                obbs_padded=out_rows, sym=out_sym, num_valid=num)


def case_statement(c, **kw):
    d = make_case(c)
    Ki = np.stack([np.linalg.inv(K) for K in d["depth_intrinsics"]])
    assert Ki.dtype == np.float32
    return statement(d["depth"], Ki, d["color_intrinsics"], d["color_size"], d["T_world_camera"], d["obbs"], d["sym"],
                     d["corners_world"], **kw)


def parity(a, b):
    """The project's parity metric: max |a - b| / max(1, |b|)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float((np.abs(a - b) / np.maximum(1.0, np.abs(b))).max()) if a.size else 0.0


def load_golden():
    z = np.load(GOLDEN)
    return z, json.loads(bytes(z["meta"]).decode())


# ---- poses for select_views: a seeded walk with turns, pauses and a few frames whose pose file holds -inf ----------------------------
def make_trajectory(seed=21, n=120):
    """{frame id: (4, 4) float64} in id order, as the reference's loader leaves it: frames with a non-finite pose are absent from the
    dict the reference sees (``finite_only``) and present, as -inf matrices, in the (n, 4, 4) array ``select_views`` is given."""
    rng = np.random.RandomState(seed)
    M = np.zeros((n, 4, 4))
    R, t = _rot(rng), rng.uniform(-1, 1, 3)
    for i in range(n):
        step = rng.randint(0, 4)
        if step == 1:
            t = t + rng.uniform(-0.06, 0.06, 3)
        elif step == 2:
            R = R @ _rot(rng, small=True)
        elif step == 3:
            t = t + rng.uniform(-0.2, 0.2, 3)
        M[i, :3, :3], M[i, :3, 3], M[i, 3, 3] = R, t, 1
    M = np.round(M, 6)
    M[[7, 8, 40, n - 1]] = -np.inf
    M[20] = M[19]                                   # an identical pose: arccos of a value that may round above 1
    return M

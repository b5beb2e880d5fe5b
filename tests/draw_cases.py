"""Helper of the drawing tests (no tests here): a float64 / integer NumPy statement of the drawing rule of parq_draw_boxes
(include/parq_hip.h; INTEGRATION.md "Drawing detections"), written from the rule and from nothing else, and the case generators.

The rule, per scene b and view t:
  base   = (x - mn) / (mx - mn) in float32, mn / mx over the 3*H*W values of the view (NaN propagates, constant view = NaN);
  corner : p_pc = R_wp^T (p_w - t_wp), p_c = R_cp p_pc + t_cp, z = p_c.z, front = z > 1e-3, uv = p_c.xy / max(z, 1e-3) * f + c,
           valid = front and 0 <= u <= w - 1 and 0 <= v <= h - 1; float64, every product and sum rounded on its own, sums left to right;
  edges  : 01 12 23 03 04 15 26 37 45 56 67 47 between valid corners, endpoints truncated to integers;
  cover  : capsule of half-width 1 around the integer segment, in integers;
  order  : boxes in index order, later over earlier; background (num_classes - 1), labels outside [0, num_classes), keep == 0 and
           m >= count[b] are skipped.
"""
import numpy as np

EDGES = ((0, 1), (1, 2), (2, 3), (0, 3), (0, 4), (1, 5), (2, 6), (3, 7), (4, 5), (5, 6), (6, 7), (4, 7))
TILE_W, TILE_H = 64, 16          # csrc/draw.hip kTileW x kTileH
CHUNK = 1024                     # csrc/draw.hip kChunk: slots examined (and at most kept in LDS) per round


# ------------------------------------------------------------------ the oracle

def segment_cover(H, W, x0, y0, x1, y1):
    """bool (H, W): the pixels the capsule of the integer segment (x0, y0) - (x1, y1) covers."""
    x0, y0, x1, y1 = (int(v) for v in (x0, y0, x1, y1))
    cover = np.zeros((H, W), bool)
    # a covered pixel is within 1 px of the segment: only the segment's bounding box grown by 1 px is evaluated
    xa, xb, ya, yb = max(min(x0, x1) - 1, 0), min(max(x0, x1) + 2, W), max(min(y0, y1) - 1, 0), min(max(y0, y1) + 2, H)
    if xa >= xb or ya >= yb:
        return cover
    y, x = np.meshgrid(np.arange(ya, yb, dtype=np.int64), np.arange(xa, xb, dtype=np.int64), indexing="ij")
    dx, dy = x1 - x0, y1 - y0
    L2 = dx * dx + dy * dy
    u = (x - x0) * dx + (y - y0) * dy
    near_a = (x - x0) ** 2 + (y - y0) ** 2 <= 1
    near_b = (x - x1) ** 2 + (y - y1) ** 2 <= 1
    cross = dx * (y - y0) - dy * (x - x0)
    cover[ya:yb, xa:xb] = near_a if L2 == 0 else np.where(u <= 0, near_a, np.where(u >= L2, near_b, cross * cross <= L2))
    return cover


def paint(H, W, segments):
    """int (H, W): the class of the last segment of ``segments`` = [(x0, y0, x1, y1, cls), ...] covering each pixel, -1 for none."""
    cls = -np.ones((H, W), np.int64)
    for x0, y0, x1, y1, c in segments:
        cls[segment_cover(H, W, x0, y0, x1, y1)] = c
    return cls


def project(cam, T_cp, T_wp, corners):
    """(u, v, z, valid) of (8, 3) float32 world corners in one view; float64, the fixed operation order of the rule."""
    cam, T_cp, T_wp, p = (np.asarray(a, np.float32).astype(np.float64) for a in (cam, T_cp, T_wp, corners))
    Rw, tw, Rc, tc = T_wp[:9].reshape(3, 3), T_wp[9:], T_cp[:9].reshape(3, 3), T_cp[9:]
    d = [p[:, i] - tw[i] for i in range(3)]
    pc = [(Rw[0, i] * d[0] + Rw[1, i] * d[1]) + Rw[2, i] * d[2] for i in range(3)]
    x, y, z = [((Rc[i, 0] * pc[0] + Rc[i, 1] * pc[1]) + Rc[i, 2] * pc[2]) + tc[i] for i in range(3)]
    zc = np.where(z > 1e-3, z, 1e-3)
    with np.errstate(all="ignore"):
        u = (x / zc) * cam[2] + cam[4]
        v = (y / zc) * cam[3] + cam[5]
        valid = (z > 1e-3) & (u >= 0.0) & (u <= cam[0] - 1.0) & (v >= 0.0) & (v <= cam[1] - 1.0)
    return u, v, z, valid


def view_segments(cam, T_cp, T_wp, corners, labels, keep, count, num_classes):
    """The drawn segments of one view in draw order: [(x0, y0, x1, y1, cls), ...]."""
    segs = []
    for m in range(corners.shape[0]):
        lab = int(labels[m])
        if lab < 0 or lab >= num_classes - 1 or (keep is not None and not keep[m]) or (count is not None and m >= int(count)):
            continue
        u, v, _, valid = project(cam, T_cp, T_wp, corners[m])
        for a, b in EDGES:
            if valid[a] and valid[b]:
                segs.append((int(np.trunc(u[a])), int(np.trunc(v[a])), int(np.trunc(u[b])), int(np.trunc(v[b])), lab))
    return segs


def normalise(view):
    """float32 (3, H, W): (x - min) / (max - min) of one view, NumPy's float32 arithmetic."""
    view = np.asarray(view, np.float32)
    with np.errstate(all="ignore"):
        mn, mx = view.min(), view.max()
        return (view - mn) / (mx - mn)


def to_uint8(x):
    """trunc(value * 255) in float32; NaN gives 0 (NumPy leaves that cast undefined, the kernel defines it)."""
    with np.errstate(all="ignore"):
        s = np.asarray(x, np.float32) * np.float32(255.0)
        return np.where(np.isnan(s), np.float32(0.0), s).astype(np.uint8)


def draw_oracle(images, camera, T_cp, T_wp, corners, labels, keep, count, colors, num_classes, uint8=False):
    """(out (B, 3, T*H, W), covered bool (B, T*H, W)) of the whole rule."""
    B, T, _, H, W = images.shape
    out = np.empty((B, 3, T * H, W), np.float32)
    covered = np.zeros((B, T * H, W), bool)
    for b in range(B):
        for t in range(T):
            img = normalise(images[b, t])
            if corners is not None and corners.shape[1] > 0:
                cls = paint(H, W, view_segments(camera[b, t], T_cp[b, t], T_wp[b, t], corners[b], labels[b], None if keep is None else keep[b],
                                                None if count is None else count[b], num_classes))
                hit = cls >= 0
                for c in range(3):
                    img[c][hit] = colors[cls[hit], c]
                covered[b, t * H:(t + 1) * H] = hit
            out[b, :, t * H:(t + 1) * H] = img
    return (to_uint8(out) if uint8 else out), covered


def art(rows):
    """bool mask of an ASCII picture ('#' = covered)."""
    return np.array([[ch == "#" for ch in row] for row in rows])


# ------------------------------------------------------------------ lattice cases: coordinates exact in float32

IDENTITY = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float32)
LATTICE_Z = 2.0                  # with fx = fy = 2 and c = 0: u = (x / 2) * 2 + 0 = x exactly


def lattice_camera(H, W):
    return np.array([W, H, 2.0, 2.0, 0.0, 0.0], np.float32)


def lattice_box(pixels):
    """(8, 3) world corners whose projections under lattice_camera + identity poses are exactly the 8 given (u, v)."""
    px = np.asarray(pixels, np.float32).reshape(8, 2)
    return np.concatenate([px, np.full((8, 1), LATTICE_Z, np.float32)], axis=1)


def flat_box(x0, y0, x1, y1):
    """A box of no depth seen frontally: its outline is the rectangle (x0, y0) - (x1, y1), its four side edges are points."""
    ring = [(x0, y0), (x1, y0), (x1, y1), (x0, y1)]
    return lattice_box(ring + ring)


def lattice_scene(H, W, boxes, labels, B=1, T=1, seed=0, images=None):
    """Arrays of a parq_draw_boxes call with identity poses and the lattice camera in every view; boxes: (M, 8, 3) shared by the
    scenes, or (B, M, 8, 3)."""
    rng = np.random.default_rng(seed)
    boxes = np.asarray(boxes, np.float32)
    if boxes.ndim == 3:
        boxes = np.broadcast_to(boxes[None], (B,) + boxes.shape).copy()
    labels = np.asarray(labels, np.int32)
    if labels.ndim == 1:
        labels = np.broadcast_to(labels[None], (B, labels.shape[0])).copy()
    if images is None:
        images = rng.standard_normal((B, T, 3, H, W)).astype(np.float32)
    cam = np.broadcast_to(lattice_camera(H, W), (B, T, 6)).copy()
    pose = np.broadcast_to(IDENTITY, (B, T, 12)).copy()
    return dict(images=images, camera=cam, T_cp=pose.copy(), T_wp=pose.copy(), corners=boxes, labels=labels)


def random_lattice_boxes(seed, M, x_lo, x_hi, y_lo, y_hi):
    """M boxes of 8 independent integer corners each in [x_lo, x_hi] x [y_lo, y_hi]: 12 arbitrary integer segments per box."""
    rng = np.random.default_rng(seed)
    px = np.stack([rng.integers(x_lo, x_hi + 1, (M, 8)), rng.integers(y_lo, y_hi + 1, (M, 8))], axis=-1)
    return np.stack([lattice_box(p) for p in px])


def exact_depth_split(value):
    """Three float32 whose float64 sum, added left to right, is exactly the float64 ``value`` (its 53 bits in 24 + 24 + 5)."""
    hi = np.float32(value)
    mid = np.float32(value - np.float64(hi))
    lo = np.float32(value - np.float64(hi) - np.float64(mid))
    assert (np.float64(hi) + np.float64(mid)) + np.float64(lo) == np.float64(value)
    return hi, mid, lo


# ------------------------------------------------------------------ random cases: real poses, generic coordinates

def _rotation(rng, amount):
    q, r = np.linalg.qr(np.eye(3) + amount * rng.standard_normal((3, 3)))
    q = q * np.sign(np.diag(r))[None, :]
    if np.linalg.det(q) < 0:
        q[:, 2] = -q[:, 2]
    return q


MARGIN = 1e-3


def box_is_generic(cams, T_cps, T_wps, corners):
    """No projected coordinate of any view within MARGIN px of an integer (image borders are integers), no depth within MARGIN of
    the 1e-3 plane.  Coordinates agree bit for bit with the kernel by construction; the margin keeps the cases meaningful for a
    cross-check that composes the poses in another order."""
    for cam, T_cp, T_wp in zip(cams, T_cps, T_wps):
        u, v, z, _ = project(cam, T_cp, T_wp, corners)
        if np.any(np.abs(z - 1e-3) < MARGIN):
            return False
        for w in (u, v):
            if not np.all(np.isfinite(w)) or np.any(np.abs(w - np.rint(w)) < MARGIN):
                return False
    return True


def random_scene(seed, B=2, T=3, H=23, W=41, M=12, num_semcls=9, focal=30.0):
    """A seeded scene of B x T views (focal length 30 px, depth 1.5 - 4 m) and M boxes per scene, classes mixed, some background,
    some keep = 0; boxes that are not generic (box_is_generic) are drawn again.  Also returns the rejection statistics."""
    rng = np.random.default_rng(seed)
    cam = np.zeros((B, T, 6), np.float32)
    cam[..., 0], cam[..., 1] = W, H
    cam[..., 2:4] = focal + rng.uniform(-1.0, 1.0, (B, T, 2))
    cam[..., 4] = (W - 1) / 2.0 + rng.uniform(-1.0, 1.0, (B, T))
    cam[..., 5] = (H - 1) / 2.0 + rng.uniform(-1.0, 1.0, (B, T))
    T_wp = np.zeros((B, T, 12), np.float32)
    T_cp = np.zeros((B, T, 12), np.float32)
    for b in range(B):
        for t in range(T):
            T_wp[b, t, :9], T_wp[b, t, 9:] = _rotation(rng, 0.08).reshape(9), 0.2 * rng.standard_normal(3)
            T_cp[b, t, :9], T_cp[b, t, 9:] = _rotation(rng, 0.05).reshape(9), 0.02 * rng.standard_normal(3)
    corners = np.zeros((B, M, 8, 3), np.float32)
    sign = np.array([(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1)], np.float64) - 0.5
    tried = rejected = 0
    for b in range(B):
        for m in range(M):
            while True:
                tried += 1
                depth = rng.uniform(1.5, 4.0)
                centre = np.array([rng.uniform(-0.6, 0.6) * depth, rng.uniform(-0.35, 0.35) * depth, depth])
                size = rng.uniform(0.2, 1.0, 3)
                ang = rng.uniform(-np.pi, np.pi)
                Ry = np.array([[np.cos(ang), 0, np.sin(ang)], [0, 1, 0], [-np.sin(ang), 0, np.cos(ang)]])
                c8 = ((sign * size) @ Ry.T + centre).astype(np.float32)
                if box_is_generic(cam[b], T_cp[b], T_wp[b], c8):
                    corners[b, m] = c8
                    break
                rejected += 1
    labels = rng.integers(0, num_semcls + 1, (B, M)).astype(np.int32)          # num_semcls = background
    keep = rng.uniform(size=(B, M)) < 0.75
    images = rng.standard_normal((B, T, 3, H, W)).astype(np.float32)
    drawable = 0
    for b in range(B):
        for m in range(M):
            ok = False
            for t in range(T):
                valid = project(cam[b, t], T_cp[b, t], T_wp[b, t], corners[b, m])[3]
                ok |= any(valid[a] and valid[c] for a, c in EDGES)
            drawable += ok
    scene = dict(images=images, camera=cam, T_cp=T_cp, T_wp=T_wp, corners=corners, labels=labels, keep=keep)
    return scene, dict(tried=tried, rejected=rejected, boxes=B * M, drawable=drawable)

"""Inputs of tests/test_gpu_parse_pred.py (data only, NumPy).

Lattice family: every float32 operation of parse_pred_kernel is exact on these inputs, so the kernel must reproduce the float64
oracle bit for bit and no pair of boxes has to be excluded.  Centres and sizes lie on a grid of 1/64 (the two pairs of GAP_PAIRS
have centres on 1/128) with |.| < 8; the ortho6d rows are a = 2 s1 e_i, b = s3 e_i + 4 s2 e_j, which Gram-Schmidt to the 24 signed
axis permutations through a real normalisation (|a| = 2, |x cross b| = 4) and a real projection (b has a component along a);
scores are multiples of 1/256, so exact ties abound.

Generic family: the generator of the g11 golden (oracle/make_golden.py::parse_case_inputs) with the number of anchors as a
parameter; for 12 anchors it draws the same numbers."""
import numpy as np

NCLS = 10                                      # 9 classes + background
TRACK_SCALE = [-7.0, 7.5, -1.0, 1.0, -7.25, 7.0]       # entries 0, 1 (x) and 4, 5 (z) are the window; strict inequalities

# Two boxes whose IoU, evaluated in float64, lies between the double threshold and the float one widened to double: extents of
# A, of B and of their intersection in units of 1/128.  0.1 < 0.10000000105 <= (double)0.1f and 0.2 < 0.20000000216 <= (double)0.2f:
# the reference (Python doubles) suppresses the lower-scored box of each pair, a comparison with 0.1f / 0.2f keeps it.
GAP_PAIRS = {0.1: ((788, 772, 640), (434, 704, 440), (321, 435, 341)), 0.2: ((664, 384, 550), (628, 638, 760), (402, 371, 497))}


def _rotations():
    rows, mats = [], []
    for i in range(3):
        for j in range(3):
            if j == i:
                continue
            for s1 in (1, -1):
                for s2 in (1, -1):
                    a, b = np.zeros(3), np.zeros(3)
                    a[i] = 2 * s1
                    b[i] = 1
                    b[j] = 4 * s2
                    x = a / 2
                    z = np.cross(x, b) / 4
                    rows.append(np.concatenate([a, b]))
                    mats.append(np.stack([x, np.cross(z, x), z], 1))
    return np.array(rows), np.array(mats)


ROT6, ROTM = _rotations()                      # 24 rows and the rotation each one stands for


def _prob_row(label, score, tie_with=None):
    p = (np.arange(NCLS) + 1) / 1024.0         # distinct, all below the smallest score (1/64)
    p[label] = score
    if tie_with is not None:
        p[list(tie_with)] = score
    return p


class _Scene:
    def __init__(self, rng):
        self.rng, self.rows, self.notes = rng, [], {}

    def box(self, lo, hi, label, score, tie_with=None, rot=None, sign=1, note=None):
        """A box with world bounds [lo, hi] under rotation `rot` (index into ROT6; random if None)."""
        lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
        r = int(self.rng.integers(24)) if rot is None else rot
        o6 = ROT6[r].copy()
        o6[3:][np.abs(o6[:3]) > 0] *= sign      # s3: the component of b along a, either sign
        size = np.abs(ROTM[r]).T @ (hi - lo)
        self.rows.append((np.concatenate([(lo + hi) / 2, size, o6, _prob_row(label, score, tie_with)])))
        if note:
            self.notes.setdefault(note, []).append(len(self.rows) - 1)

    def arrays(self, Q):
        X = np.array(self.rows)
        assert X.shape[0] == Q, (X.shape, Q)
        perm = self.rng.permutation(Q)         # the special boxes land anywhere in [0, Q), beyond index 256 too
        X = X[perm]
        inv = np.argsort(perm)
        notes = {k: [int(inv[i]) for i in v] for k, v in self.notes.items()}
        return X, notes


def _fillers(sc, n, background=0.45):
    """Random lattice boxes in x < -0.75: they overlap each other at random and never touch the special boxes (x > 0)."""
    rng = sc.rng
    for _ in range(n):
        c = np.array([rng.integers(-6 * 64, -96 + 1), rng.integers(-480, 481), rng.integers(-480, 481)]) / 64.0
        half = rng.integers(8, 49, 3) / 64.0                        # world extents 1/4 .. 3/2
        label = NCLS - 1 if rng.random() < background else int(rng.integers(0, NCLS - 1))
        sc.box(c - half, c + half, label, int(rng.integers(4, 256)) / 256.0, sign=int(rng.choice([1, -1])))


def _special(sc):
    """The edge cases, each in a region of its own at x > 0 (no overlap between groups)."""
    u = 1 / 64.0
    cells = [np.array([0.25 + 3.25 * i, -7.75 + 3.0 * j, -1.25 + 3.25 * k]) for k in range(3) for j in range(5) for i in range(2)]
    cell = iter(cells)
    # IoU exactly 0.1 = (1/8) / (11/16 + 11/16 - 1/8), and the neighbouring grid point above it
    for dz, note in ((0, "iou_on_0.1"), (u, "iou_above_0.1")):
        o = next(cell)
        sc.box(o, o + [.5, .5, 2.75], 1, .75, note=note)
        sc.box(o, o + [.5, 2.75, .5 + dz], 1, .5, note=note)
    # IoU exactly 0.2 = (1/8) / (3/8 + 3/8 - 1/8), and the neighbouring grid point above it
    for dz, note in ((0, "iou_on_0.2"), (u, "iou_above_0.2")):
        o = next(cell)
        sc.box(o, o + [.5, .5, 1.5], 2, .75, note=note)
        sc.box(o, o + [.5, 1.5, .5 + dz], 2, .5, note=note)
    # tied scores: an overlapping pair (the visit order decides which survives) and a pair apart
    o = next(cell)
    sc.box(o, o + 1.0, 3, .625, note="tie_overlap")
    sc.box(o + .125, o + 1.125, 3, .625, note="tie_overlap")
    sc.box(o + [0, 1.5, 0], o + [1, 2.5, 1], 3, .625, note="tie_apart")
    sc.box(o + [0, 1.5, 1.5], o + [1, 2.5, 2.5], 3, .625, note="tie_apart")
    # two largest class probabilities equal: the first wins (label 2, not 5) - decides what the identical boxes below suppress
    o = next(cell)
    sc.box(o, o + 1.0, 2, .875, tie_with=(5,), note="class_tie")
    sc.box(o, o + 1.0, 5, .8125, note="class_tie")
    sc.box(o, o + 1.0, 2, .78125, note="class_tie")
    # background tied with a class (the class comes first: a candidate), all ten equal (label 0), background alone on top
    o = next(cell)
    sc.box(o, o + .5, 3, .5, tie_with=(NCLS - 1,), note="background_tie")
    sc.box(o + [0, 1, 0], o + [.5, 1.5, .5], 0, .5, tie_with=range(NCLS), note="background_tie")
    sc.box(o + [0, 2, 0], o + [.5, 2.5, .5], NCLS - 1, .96875, note="background_top")
    # zero-size boxes on top of each other (IoU 0 / 0), flat boxes of zero volume, a point inside a box
    o = next(cell)
    for s in (.75, .5, .25):
        sc.box(o + .5, o + .5, 4, s, note="zero_size")
    sc.box(o + [0, 1.5, 0], o + [1, 2.5, 0], 4, .75, note="zero_size")
    sc.box(o + [0, 1.5, 0], o + [1, 2.5, 0], 4, .5, note="zero_size")
    sc.box(o + [1.5, 0, 0], o + [2.5, 1, 1], 4, .75, note="zero_size")
    sc.box(o + [2, .5, .5], o + [2, .5, .5], 4, .5, note="zero_size")
    # a box containing another: IoU 8/27 (suppressed) and 1/64 (kept)
    o = next(cell)
    sc.box(o, o + 1.5, 6, .9375, note="contains")
    sc.box(o + .25, o + 1.25, 6, .5, note="contains")
    o = next(cell)
    sc.box(o, o + 2.0, 6, .9375, note="contains")
    sc.box(o + .5, o + 1.0, 6, .5, note="contains")
    # identical boxes of different classes: both kept in the visualisation variant, one in the evaluation variant
    o = next(cell)
    sc.box(o, o + [1, 2, .5], 7, .75, note="other_class")
    sc.box(o, o + [1, 2, .5], 8, .5, note="other_class")
    # centres exactly on the window (invalid: the inequalities are strict) and one grid point inside it
    tx0, tx1, tz0, tz1 = TRACK_SCALE[0], TRACK_SCALE[1], TRACK_SCALE[4], TRACK_SCALE[5]
    h = 1 / 16.0
    for n, (cx, cz) in enumerate(((tx1, 0.), (tx0, 0.), (7.25, tz0), (7.25, tz1))):
        for m, (ex, ez) in enumerate(((0, 0), (-u if cx == tx1 else (u if cx == tx0 else 0), u if cz == tz0 else (-u if cz == tz1 else 0)))):
            c = np.array([cx + ex, -6.0 + n + .25 * m, cz + ez])
            sc.box(c - h, c + h, 5, .5, note="on_window" if m == 0 else "inside_window")
    # IoU between the double and the float threshold (GAP_PAIRS), in z < -1.6
    for thr, org in ((0.1, np.array([0., -8., -8.])), (0.2, np.array([0., .5, -8.]))):
        a, b, c = (np.array(v) / 128.0 for v in GAP_PAIRS[thr])
        sc.box(org, org + a, 1, .75, note="gap_%s" % thr)
        sc.box(org + a - c, org + a - c + b, 1, .5, note="gap_%s" % thr)


def lattice_scene(kind, Q, seed):
    """kind: "full" (edge cases + random lattice boxes; Q >= 255), "tiny" (Q = 1: one box; Q = 2: a tied overlapping pair),
    "background" (no candidate), "single" (one candidate).  Returns (Q, 25) float64 rows [centre | size | rot6 | prob] and notes."""
    sc = _Scene(np.random.default_rng(seed))
    if kind == "full":
        _special(sc)
        _fillers(sc, Q - len(sc.rows))
    elif kind == "tiny":
        sc.box([0, 0, 0], [1, 1, 1], 3, .5)
        if Q == 2:
            sc.box([.125, 0, 0], [1.125, 1, 1], 3, .5)
    else:
        _fillers(sc, Q, background=1.0)
    X, notes = sc.arrays(Q)
    if kind == "single":
        X[Q // 2, 12:] = _prob_row(4, .5)
        X[Q // 2, :3] = [-2.0, 0.0, 1.0]
    return X, notes


def lattice_case(Q, B, seed=7):
    kinds = ["full" if Q >= 255 else "tiny"] + ["background", "single"][:B - 1]
    scenes = [lattice_scene(k, Q, seed + 13 * n) for n, k in enumerate(kinds)]
    X = np.stack([s[0] for s in scenes]).astype(np.float32)
    assert np.array_equal(X.astype(np.float64), np.stack([s[0] for s in scenes]))        # everything is a float32 already
    return dict(center=X[..., 0:3].copy(), size=X[..., 3:6].copy(), rot6=X[..., 6:12].copy(), prob=X[..., 12:].copy()), scenes[0][1], kinds


def generic_inputs(seed, B, Q, anchors=12):
    """oracle/make_golden.py::parse_case_inputs with the number of anchors as a parameter (same draws for 12)."""
    rng = np.random.RandomState(seed)
    anc = rng.uniform(-1.2, 1.2, (B, anchors, 3)) * np.array([1.0, 0.5, 1.0]) + np.array([0.0, -0.5, 1.0])
    which = rng.randint(0, anchors, (B, Q))
    center = np.take_along_axis(anc, which[..., None].repeat(3, -1), 1) + rng.normal(0, 0.08, (B, Q, 3))
    center[:, :6] += rng.uniform(-3, 3, (B, 6, 3))
    size = rng.uniform(0.3, 0.9, (B, Q, 3))
    rot6 = rng.normal(0, 1, (B, Q, 6))
    logits = rng.normal(0, 1.5, (B, Q, 10))
    prob = np.exp(logits) / np.exp(logits).sum(-1, keepdims=True)
    return {k: v.astype(np.float32) for k, v in dict(center=center, size=size, rot6=rot6, prob=prob).items()}


GENERIC_TRACK_SCALE = [-1.5, 1.5, -2, 1, 0, 2]
# (seed, Q, anchors): the smallest |IoU - threshold| of the float64 oracle is at least 2e-5 in both variants (asserted by the test;
# 1.4e-4 / 1.9e-4, 3.9e-4 / 2.1e-4, 3.1e-4 / 9.2e-5 for the first three; seeds 43 at Q = 512 and 44 at Q = 1024 fall under 1e-5)
GENERIC_CASES = [(42, 257, 12), (42, 512, 12), (46, 1024, 12)]

"""The device matcher's rules as NumPy statements (include/parq_hip.h parq_set_match), and the seeded cases of its tests
(test_set_match_cpu.py, test_gpu_set_match.py).

``cost_statement`` is part a of the entry: float32 softmax, L1 distances, m = -(cost_bbox * l1 - cost_class * prob), near = l1 < ratio,
every operation one float32 rounding in the written order (``dtype=np.float64``: the same expression in float64, the reference of
the kernel's cost error).  ``match_statement`` is parts b-d on a GIVEN cost: ``assign_statement`` (tests/scene_tracks_cases.py) for the
assignment, the hash, the cap rule, one box per prediction, the punish mask of the last box, and pair_coef / row_weight in float32.
The kernel must reproduce ``match_statement`` bit for bit on its own cost."""
import numpy as np

from scene_tracks_cases import assign_statement

COST_CLASS, COST_BBOX, RATIO, MAX_PADDING = 2.0, 0.25, 0.2, 10
GOLDEN = 0x9E3779B9


# ---- the hash -----------------------------------------------------------------------------------------------------------------
def mix32(h):
    """uint32 -> uint32 on an array (wrapping products)."""
    h = np.asarray(h, np.uint32).copy()
    h ^= h >> np.uint32(16)
    h *= np.uint32(0x7FEB352D)
    h ^= h >> np.uint32(15)
    h *= np.uint32(0x846CA68B)
    h ^= h >> np.uint32(16)
    return h


def match_keys(seed, step, k, b, j, qs):
    """key = H(seed_lo, seed_hi, step, k, b, j, q) for every q of `qs`: h = 0x9e3779b9; for each word w: h = mix((h ^ w) + 0x9e3779b9)."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    h = np.full(len(qs), GOLDEN, np.uint32)
    with np.errstate(over="ignore"):
        for w in (seed & 0xFFFFFFFF, seed >> 32, int(step) & 0xFFFFFFFF, k, b, j):
            h = mix32((h ^ np.uint32(w)) + np.uint32(GOLDEN))
        return mix32((h ^ np.asarray(qs, np.uint32)) + np.uint32(GOLDEN))


# ---- part a: the cost -----------------------------------------------------------------------------------------------------------
def cost_statement(logits, coord, t_center, t_label, t_count, cost_class=COST_CLASS, cost_bbox=COST_BBOX, ratio=RATIO, dtype=np.float32):
    """(m (I,B,Q,nmax) of `dtype`, near (I,B,Q,nmax) bool); columns j >= t_count[b] are 0 / False."""
    f = dtype
    lg, xyz, tc = (np.asarray(a, np.float32).astype(f) for a in (logits, coord, t_center))
    I, B, Q, ncls = lg.shape
    nmax = tc.shape[1]
    cc, cb, rt = f(np.float32(cost_class)), f(np.float32(cost_bbox)), f(np.float32(ratio))
    e = np.exp(lg - lg.max(-1, keepdims=True))
    s = np.zeros((I, B, Q), f)
    for c in range(ncls):                                                    # the sum in index order
        s = s + e[..., c]
    m, near = np.zeros((I, B, Q, nmax), f), np.zeros((I, B, Q, nmax), bool)
    for b in range(B):
        for j in range(int(t_count[b])):
            lab = int(t_label[b, j])
            prob = e[:, b, :, lab] / s[:, b] if 0 <= lab < ncls else np.zeros((I, Q), f)
            d = np.abs(xyz[:, b] - tc[b, j])
            l1 = (d[..., 0] + d[..., 1]) + d[..., 2]
            m[:, b, :, j] = -(cb * l1 - cc * prob)
            near[:, b, :, j] = l1 < rt
    return m, near


# ---- parts b-d: the matching on a given cost ---------------------------------------------------------------------------------------
def match_segment(m_seg, near_seg, seed, step, k, b, max_padding=MAX_PADDING):
    """One (iteration, scene): (row_to_col (Q,), g (Q,), punish (Q,) bool, chosen (Q, n) bool) of the (Q, n) cost and near matrices."""
    Q, n = m_seg.shape
    r2c = assign_statement(m_seg) if n > 0 else -np.ones(Q, np.int32)
    extra = -np.ones(Q, np.int32)
    punish = np.ones(Q, bool)
    chosen = np.zeros((Q, n), bool)
    for j in range(n):
        nb = np.nonzero(near_seg[:, j])[0]
        if len(nb) > max_padding:                                            # the max_padding neighbours of smallest (key, q)
            keys = match_keys(seed, step, k, b, j, nb)
            nb = nb[np.lexsort((nb, keys))[:max_padding]]
        chosen[nb, j] = True
        extra[nb[extra[nb] < 0]] = j                                         # the lowest box that chose q
        if j == n - 1:
            punish = ~near_seg[:, j] | chosen[:, j]
    g = np.where(r2c >= 0, r2c, extra).astype(np.int32)
    return r2c.astype(np.int32), g, punish, chosen


def match_statement(m, near, t_count, seed, step, max_padding=MAX_PADDING):
    """All outputs of parq_set_match for the dense cost m and near (I,B,Q,nmax): row_to_col (I,B,Q), pairs (4, P), pair_coef (P,),
    row_weight (P,), stats (I*B + 1,), and punish / chosen for the tests of the rule itself."""
    m, near = np.asarray(m, np.float32), np.asarray(near).astype(bool)
    I, B, Q, nmax = m.shape
    f = np.float32
    r2c, g = -np.ones((I, B, Q), np.int32), -np.ones((I, B, Q), np.int32)
    punish, chosen = np.ones((I, B, Q), bool), np.zeros((I, B, Q, nmax), bool)
    for k in range(I):
        for b in range(B):
            n = int(t_count[b]) if 0 <= int(t_count[b]) <= nmax else 0
            r2c[k, b], g[k, b], punish[k, b], chosen[k, b, :, :n] = match_segment(m[k, b, :, :n], near[k, b, :, :n], seed, step, k, b, max_padding)
    cnt = (g >= 0).sum(-1)
    valid = cnt > 0
    vbs = int(valid.sum())
    coef, rw = np.zeros((I, B), f), np.zeros((I, B, Q), f)
    if vbs > 0:
        coef[valid] = f(1.0) / (cnt[valid].astype(f) * f(vbs))
        pm = punish.astype(f)
        ps = pm.sum(-1, keepdims=True)
        rw = ((np.divide(pm, ps, out=np.zeros_like(pm), where=ps > 0) * valid[..., None].astype(f)) / f(vbs)).astype(f)
    kk, bb, qq = np.meshgrid(np.arange(I), np.arange(B), np.arange(Q), indexing="ij")
    pairs = np.stack([kk, bb, qq, g]).reshape(4, -1).astype(np.int32)
    return dict(row_to_col=r2c, g=g, pairs=pairs, pair_coef=np.repeat(coef.reshape(-1), Q).astype(f), row_weight=rw.reshape(-1),
                stats=np.concatenate([cnt.reshape(-1), [vbs]]).astype(np.int32), punish=punish, chosen=chosen, cnt=cnt)


def segment_pairs(st, k, b):
    """(queries, boxes) of one segment of a match_statement result, in query order: the host matcher's indices[b]."""
    g = st["g"][k, b]
    p = np.nonzero(g >= 0)[0]
    return p, g[p]


# ---- the kernel's cases ---------------------------------------------------------------------------------------------------------
# (I, B, Q, ncls, nmax), boxes per scene
SHAPES = {"more_boxes": ((1, 1, 8, 2, 12), [12]), "odd_q": ((2, 3, 70, 10, 5), [1, 5, 3]), "cfg4": ((8, 4, 256, 10, 12), [12, 12, 12, 12]),
          "wide": ((1, 2, 300, 4, 20), [20, 7])}
VARIANTS = ("none", "last", "first")
CLUSTER = 30                     # reference points put around an over-full box


def case_max_padding(shape):
    """10 as in the reference; Q = 8 cannot hold 30 neighbours, so there every point is a neighbour and the cap is 3."""
    return MAX_PADDING if SHAPES[shape][0][2] >= CLUSTER else 3


def _ball(rng, n, radius):
    """n offsets of L1 norm below `radius`."""
    d = rng.uniform(-1, 1, (n, 3))
    return d / np.abs(d).sum(1, keepdims=True) * rng.uniform(0, radius, (n, 1))


def kernel_case(shape, variant, seed=0):
    """Inputs of parq_set_match.  Box centres sit on a jittered lattice (L1 distance between two centres > 1, so no point is near
    two boxes unless the variant says so); every box gets 0-2 neighbours; `last` puts CLUSTER points within 0.05 of the last box
    of every scene, `first` moves box 1 to 0.1 of box 0 and puts CLUSTER points within 0.04 of their midpoint (near both)."""
    (I, B, Q, ncls, nmax), counts = SHAPES[shape]
    rng = np.random.RandomState(7000 + 100 * list(SHAPES).index(shape) + 10 * VARIANTS.index(variant) + seed)
    logits = rng.normal(0, 2, (I, B, Q, ncls)).astype(np.float32)
    cells = np.stack(np.meshgrid(*[np.arange(4)] * 3, indexing="ij"), -1).reshape(-1, 3)
    t_center = np.stack([cells[rng.permutation(64)[:nmax]] * 1.5 - 2.25 + rng.uniform(-0.2, 0.2, (nmax, 3)) for _ in range(B)]).astype(np.float32)
    t_label = rng.randint(0, ncls, (B, nmax)).astype(np.int32)
    if shape == "wide":
        t_label[0, 1], t_label[1, 2] = -1, ncls + 3                          # labels outside [0, ncls): probability 0
    if variant == "first":
        for b in range(B):
            if counts[b] >= 2:
                t_center[b, 1] = t_center[b, 0] + np.float32([0.1, 0, 0])
    coord = rng.uniform(-9, -6, (I, B, Q, 3)).astype(np.float32)               # far from every box
    npts = min(CLUSTER, Q)
    for k in range(I):
        for b in range(B):
            order, used = rng.permutation(Q), 0
            if variant != "none":
                j = counts[b] - 1 if variant == "last" else 0
                mid = t_center[b, j] if (variant == "last" or counts[b] < 2) else 0.5 * (t_center[b, 0] + t_center[b, 1])
                coord[k, b, order[:npts]] = mid + _ball(rng, npts, 0.05 if variant == "last" else 0.04)
                used = npts
            for j in range(counts[b]):
                r = min(int(rng.randint(0, 3)), Q - used)
                coord[k, b, order[used:used + r]] = t_center[b, j] + _ball(rng, r, 0.15)
                used += r
    return dict(I=I, B=B, Q=Q, ncls=ncls, nmax=nmax, logits=logits, coord=coord, t_center=t_center, t_label=t_label,
                t_count=np.asarray(counts, np.int32), max_padding=case_max_padding(shape))


def over_full(near, t_count, max_padding):
    """(I, B, nmax) bool: boxes with more neighbours than the cap."""
    cnt = np.asarray(near).sum(2)
    return (cnt > max_padding) & (np.arange(near.shape[3])[None, None] < np.asarray(t_count)[None, :, None])


# ---- cases for the comparison with the host matcher -------------------------------------------------------------------------------
ROBUST_SEEDS = (1, 2, 3)         # scanned on the CPU (test_set_match_cpu.py asserts it): +-1e-5 on the cost leaves scipy's assignment


def host_case(seed, I=2, B=2, Q=64, ncls=10, nbox=(5, 9), capped=False):
    """Decoder outputs as NumPy dicts and targets for parq_amd.loss: boxes of synth.make_boxes in the local frame of a synthetic
    T_world_local, 0-3 reference points near each box (`capped`: 14 around the last box of scene 0 and 13 around box 0 of scene 1)."""
    import torch
    from parq_amd import Obb3D, Pose, synth
    from parq_amd.loss import parse_target
    rng = np.random.RandomState(9100 + seed)
    obbs, sym = synth.make_boxes(9200 + seed, B, max(nbox), max_box=16)
    for b in range(B):
        obbs[b, nbox[b]:], sym[b, nbox[b]:] = -1, -1
    T_wl = synth.make_geometry(9300 + seed, B, 2, 8, 8)[3]
    targets = parse_target(Obb3D(torch.from_numpy(obbs)), Pose(torch.from_numpy(T_wl)))
    outs = []
    for k in range(I):
        coord = rng.uniform(-9, -6, (B, Q, 3)).astype(np.float32)
        for b in range(B):
            ctr = targets[b]["center"].numpy()
            order, used = rng.permutation(Q), 0
            for j in range(nbox[b]):
                r = int(rng.randint(0, 4))
                if capped and (b, j) in ((0, nbox[0] - 1), (1, 0)):
                    r = 14 - b
                coord[b, order[used:used + r]] = ctr[j] + _ball(rng, r, 0.15)
                used += r
        outs.append({"pred_logits": rng.normal(0, 1.5, (B, Q, ncls)).astype(np.float32), "coord_pos": coord,
                     "center_unnormalized": rng.normal(0, 1.5, (B, Q, 3)).astype(np.float32),
                     "size_unnormalized": (rng.uniform(0.2, 1.2, (B, Q, 3))).astype(np.float32),
                     "ortho6d": rng.normal(0, 1, (B, Q, 6)).astype(np.float32)})
    return outs, obbs, T_wl, sym, targets


def host_case_cost(outs, targets):
    """cost_statement on a host_case: (m, near, t_count)."""
    B = len(targets)
    counts = np.asarray([len(t["labels"]) for t in targets], np.int32)
    nmax = int(counts.max())
    tc, tl = np.zeros((B, nmax, 3), np.float32), np.zeros((B, nmax), np.int32)
    for b, t in enumerate(targets):
        tc[b, :counts[b]], tl[b, :counts[b]] = t["center"].numpy(), t["labels"].numpy()
    m, near = cost_statement(np.stack([o["pred_logits"] for o in outs]), np.stack([o["coord_pos"] for o in outs]), tc, tl, counts)
    return m, near, counts

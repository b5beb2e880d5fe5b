"""Inputs of tests/test_gpu_set_loss_kernel.py (data only, NumPy): decoder outputs, padded targets and hand-built matched pairs for
parq_set_loss_flags, so that any number of pairs P can be chosen without the matcher."""
import numpy as np

W4 = [2.0, 1.5, 0.7, 1.2]
# rows of the pair list that carry an edge case when `edges` is set and P is large enough (index into the pairs)
EDGE_EQUAL, EDGE_SMALL_A, EDGE_LARGE_A, EDGE_NEAR_PARALLEL = 0, 1, 2, 3


def _rotation(rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 2] = -q[:, 2]
    return q


def make_case(I, B, Q, ncls, nmax, P, seed, edges=True, turn=True):
    """Returns a dict: outputs (logits, center, size, o6), targets (t_center, t_size, t_rot, t_label), pairs (4, P) int32 with
    distinct (k, b, q), coef (P), row_weight (I, B, Q), class_weight, w4, sym (B, nmax) int32 with classes 0..3 all present."""
    rng = np.random.default_rng(seed)
    f = lambda a: np.ascontiguousarray(a, np.float32)
    out = dict(logits=f(rng.normal(size=(I, B, Q, ncls))), center=f(rng.normal(size=(I, B, Q, 3)) * 2),
               size=f(rng.random((I, B, Q, 3)) + 0.2), o6=f(rng.normal(size=(I, B, Q, 6))))
    tg = dict(t_center=f(rng.normal(size=(B, nmax, 3)) * 2), t_size=f(rng.random((B, nmax, 3)) + 0.2),
              t_rot=f(np.stack([[_rotation(rng) for _ in range(nmax)] for _ in range(B)])),
              t_label=rng.integers(0, ncls - 1, (B, nmax)).astype(np.int32))
    sym = (np.arange(B * nmax).reshape(B, nmax) % 4).astype(np.int32)
    rows = rng.permutation(I * B * Q)[:P]                                   # distinct (k, b, q), drawn without replacement
    pairs = np.stack([rows // (B * Q), rows // Q % B, rows % Q, rng.integers(0, nmax, P)]).astype(np.int32)
    # matched rows predict T Ry(psi) E as a = |a| x, b = |b| y + mu a.  E turns by 25 .. 80 degrees about an axis perpendicular to
    # y, so R is never close to a symmetry candidate T Ry(theta) and the rotation gradient of a row is not the small difference of
    # large parts, which any fp32 evaluation returns with its relative error blown up.  psi (`turn`; 0 without symmetry classes)
    # lies within 3.5 degrees of a candidate of the box's class, a different one from pair to pair: every candidate gets chosen,
    # and the runner-up (5 degrees away at the closest, in class 3) stays clear of the minimum.
    folds = {1: 2, 2: 4, 3: 36}
    for j in range(P):
        k, b, q, g = pairs[:, j]
        phi, ang = rng.uniform(0, 2 * np.pi), np.radians(rng.uniform(25, 80))
        ax = np.array([np.cos(phi), 0.0, np.sin(phi)])
        K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
        m = folds.get(int(sym[b, g]), 0) if turn else 0
        psi = 2 * np.pi * rng.integers(0, m) / m + np.radians(rng.uniform(-3.5, 3.5)) if m else 0.0
        Ry = np.array([[np.cos(psi), 0, np.sin(psi)], [0, 1, 0], [-np.sin(psi), 0, np.cos(psi)]])
        R = tg["t_rot"][b, g].astype(np.float64) @ Ry @ (np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * K @ K)
        a = R[:, 0] * rng.uniform(0.3, 3.0)
        out["o6"][k, b, q] = f(np.concatenate([a, R[:, 1] * rng.uniform(0.3, 3.0) + rng.uniform(-1, 1) * a]))
    seg = pairs[0] * B + pairs[1]
    cnt = np.bincount(seg, minlength=I * B)
    valid_bs = max(1, int((cnt > 0).sum()))
    coef = f(1.0 / (cnt[seg] * valid_bs))
    punish = rng.random((I, B, Q)) < 0.8
    punish[..., 0] = True
    rw = punish / punish.sum(-1, keepdims=True) / valid_bs
    if edges:
        sat = out["logits"][:, :, ::5]                                      # saturated rows: one logit near +80, one near -80
        hi_lo = np.argsort(rng.random(sat.shape), -1)[..., :2]
        np.put_along_axis(sat, hi_lo, f(np.array([80.0, -80.0]) + rng.normal(size=sat.shape[:-1] + (2,))), -1)
        out["logits"][:, :, ::5] = sat
        rw[I - 1, B - 1] = 0.0                                              # an (iteration, scene) whose rows all have weight 0
        tg["t_label"][0, 0], tg["t_label"][B - 1, nmax - 1] = -1, ncls + 3  # both act as background
        if P > 8:                                                           # ... and pairs 4 and 5 really carry such labels
            tg["t_label"][pairs[1, 4], pairs[3, 4]], tg["t_label"][pairs[1, 5], pairs[3, 5]] = -1, ncls + 3
        if P > 8:
            k, b, q, g = pairs[:, EDGE_EQUAL]
            out["center"][k, b, q, 0] = tg["t_center"][b, g, 0]             # residual exactly zero: gradient component 0
            out["size"][k, b, q, 1] = tg["t_size"][b, g, 1]
            for e, scale in ((EDGE_SMALL_A, 1e-3), (EDGE_LARGE_A, 1e3)):
                k, b, q, g = pairs[:, e]
                a = out["o6"][k, b, q, :3].astype(np.float64)
                out["o6"][k, b, q, :3] = f(a / np.linalg.norm(a) * scale)
            k, b, q, g = pairs[:, EDGE_NEAR_PARALLEL]
            a = out["o6"][k, b, q, :3].astype(np.float64)
            n = np.cross(a, [0.3, -0.5, 0.8])
            n = n / np.linalg.norm(n) * np.linalg.norm(a)
            out["o6"][k, b, q, 3:] = f(1.3 * (np.cos(np.radians(5)) * a + np.sin(np.radians(5)) * n))      # 5 degrees from a
    cw = np.ones(ncls, np.float32)
    cw[ncls - 1] = 0.1
    return dict(outputs=out, targets=tg, pairs=pairs, coef=coef, row_weight=f(rw), class_weight=cw, w4=W4, sym=sym)

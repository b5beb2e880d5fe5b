"""Hand-placed inputs of the project-and-sample backward tests (tests/test_sample_bwd_cpu.py, tests/test_gpu_sample_bwd.py) and the
float64 statements the device results are judged against.

The inputs are NumPy only.  Every placed query sits at pixel coordinates that are exact: the poses of the placed views are the
identity, fx = fy = 1, cx = cy = 0, the scale box is [0, 8] on each axis and ref = (x / 8, y / 8, z / 8) in float32 with x, y, z
short dyadic numbers, so P = 8 ref, u = x / z and v = y / z carry no rounding in float64 (kernel and oracle alike).  "Mixed" views
add poses from synth.make_geometry; whatever lands in them is generic, and the generator keeps generic points MARGIN pixels away
from every lattice line (hence from every validity limit, which are integers) in every view.

The families (one tag per query, `case["family"]`):
  lattice   u in {0, interior, w-1} x v in {0, interior, h-1}: valid, weights exactly 1 and 0
  band      u in (-1, 0) or (w-1, w), v likewise, and both at once: sampled with 1 or 2 corners, not valid in a (w, h) camera
  outside   u = -1 exactly (sampled, all weights zero), u = w exactly, u < -1, u > w (and the same in v): contribute nothing
  camgrid   a view whose camera is (w + 3, h + 2): u in (w-1, w+2] is valid there and counts in the denominator, sampled partly or not
  clamp     z = 2^-9 (in front, gains ~500 per unit), z = 2^-11 (clamped to eps: sampled, not valid, dz = 0), z < 0 (|u| ~ 1e3 .. 1e6)
  novalid   every view of the query lies in a band: the denominator is max(0, 1)
  generic   uniform points, off the lattice by MARGIN in every view ("mixed": with rotated views)
  pileup    many queries sharing a few footprints

`gref_excluded` marks the queries whose coordinate gradient is not judged: at an exact integer coordinate the bilinear sample has a
kink, where the kernel takes the right-hand derivative (as grid_sample's backward does) and the explicit oracle the sign(0) = 0
subgradient.  These are the lattice family, the exact u = -1 / u = w (v = -1 / v = h) members of `outside`, and the clamp query
that sits on the principal point (0, 0), an exact pixel.  Their forward value and token gradient are judged like everyone's.
"""
import numpy as np

from parq_amd import synth

SCALE = [0.0, 8.0, 0.0, 8.0, 0.0, 8.0]
MARGIN = 2.0 ** -6
EPS = 1e-3                                         # Camera.project's clamp as the float64 oracle applies it.  The kernels clamp at the
#                                                    float32 value of 1e-3, as a float32 run of the reference does: 4.7e-8 more.  No
#                                                    depth here lies between the two, and a clamped point that is sampled sits at
#                                                    u, v < 1, where the two quotients differ by less than 5e-8 px.
FAMILIES = ("lattice", "band", "outside", "camgrid", "clamp", "novalid", "generic", "pileup")
IDENTITY = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float64)
TILE, ROUND, CHUNK = 8, 256, 1024                  # sample_det_gather_kernel: pixel tile, compaction round, kDetList

#                  id        B  V  h  w   C     Q     token type
SHAPES = {"edges": (2, 3, 5, 6, 64, 48, "f32"), "seams": (1, 2, 9, 17, 64, 300, "f32"), "chunks": (1, 1, 9, 17, 64, 1100, "f32"),
          "views17": (1, 17, 5, 6, 64, 24, "f32"), "wide": (1, 2, 5, 6, 1024, 16, "f32"),
          "tok16-f16": (1, 3, 5, 6, 256, 48, "f16"), "tok16-bf16": (1, 3, 5, 6, 256, 48, "bf16")}
CASE_IDS = tuple(SHAPES)
FP32_CASE_IDS = tuple(k for k, s in SHAPES.items() if s[6] == "f32")


def _camera(B, V, h, w, big_view=None):
    cam = np.zeros((B, V, 6), np.float32)
    cam[..., 0], cam[..., 1], cam[..., 2], cam[..., 3] = w, h, 1.0, 1.0
    if big_view is not None:
        cam[:, big_view, 0], cam[:, big_view, 1] = w + 3, h + 2
    return cam


def _rotated_poses(seed, B, V, h, w):
    """T_camera_local (B, V, 12) float64 of synth.make_geometry's float32 pose stacks: T_cp o (inv(T_wp) o T_wl)."""
    _, T_cp, T_wp, T_wl = synth.make_geometry(seed, B, V, h, w)
    split = lambda T: (T[..., :9].astype(np.float64).reshape(T.shape[0], T.shape[1], 3, 3), T[..., 9:].astype(np.float64))
    (Rc, tc), (Rw, tw), (Rl, tl) = split(T_cp), split(T_wp), split(T_wl)
    Ri = np.swapaxes(Rw, -1, -2)
    ti = -(Ri @ tw[..., None])[..., 0]
    Rm, tm = Ri @ Rl, ti + (Ri @ tl[..., None])[..., 0]
    R, t = Rc @ Rm, tc + (Rc @ tm[..., None])[..., 0]
    return np.concatenate([R.reshape(B, V, 9), t], -1)


def _poses(seed, B, V, h, w, rotated_from):
    """Identity for the views below `rotated_from`, make_geometry's poses from there on."""
    T = np.broadcast_to(IDENTITY, (B, V, 12)).copy()
    if rotated_from < V:
        T[:, rotated_from:] = _rotated_poses(seed, B, V, h, w)[:, rotated_from:]
    return T


def project(ref, T_cl, cam):
    """Pose.transform + Camera.project in float64 (NumPy): p2d (B,V,Q,2), z (B,V,Q), valid (B,V,Q)."""
    P = ref.astype(np.float64) * 8.0                                              # SCALE: lo = 0, hi - lo = 8
    R, t = T_cl[..., :9].reshape(T_cl.shape[:2] + (3, 3)), T_cl[..., 9:]
    pc = np.einsum("bqj,bvij->bvqi", P, R) + t[:, :, None, :]
    z = pc[..., 2]
    zc = np.maximum(z, EPS)
    c = cam.astype(np.float64)
    p2d = pc[..., :2] / zc[..., None] * c[:, :, None, 2:4] + c[:, :, None, 4:6]
    size = c[:, :, None, :2]
    valid = (z > EPS) & np.all((p2d >= 0) & (p2d <= size - 1), -1)
    return p2d, z, valid


def footprint(p2d, h, w):
    """floor corner (x0, y0) as float64 and whether the view samples at all (a corner can be in range), as the kernels decide it."""
    fx0, fy0 = np.floor(p2d[..., 0]), np.floor(p2d[..., 1])
    on = (fx0 >= -1) & (fx0 <= w - 1) & (fy0 >= -1) & (fy0 <= h - 1)
    return fx0, fy0, on


def lattice_distance(p2d):
    """Distance of every pixel coordinate to the nearest lattice line, minimum over (u, v)."""
    return np.abs(p2d - np.round(p2d)).min(-1)


def _ref_of(x, y, z):
    r = np.array([x / 8.0, y / 8.0, z / 8.0], np.float64)
    assert np.all(r.astype(np.float32).astype(np.float64) == r), (x, y, z)        # exactly representable: no rounding anywhere
    return r.astype(np.float32)


def _edges_placed(h, w):
    """(family, x, y, z, intended (u, v) in the identity views or None, g_ref excluded) of the placed scene of `edges`."""
    xi, yi = w // 2, h // 2
    q = []
    add = lambda fam, u, v, excl=False: q.append((fam, u, v, 1.0, (u, v), excl))
    for v in (0, yi, h - 1):
        for u in (0, xi, w - 1):
            add("lattice", float(u), float(v), True)
    # (the right and the bottom band's masked corners stand in at tokens (3, 0), (0, 2): nothing else touches those)
    for u, v in ((-0.25, 1.5), (w - 0.5, 3.5), (0.5, -0.5), (1.5, h - 0.75),                       # one band
                 (-0.5, -0.25), (w - 0.75, -0.75), (-0.75, h - 0.5), (w - 0.5, h - 0.25)):         # corner bands
        add("band", u, v)
    # (the oracle's float64 round trip through the normalised grid can move u = -1 to -1 + 2e-16, a weight of 2e-16 on column 0:
    # the query sits beside rows that the left band touches anyway, so no row's "exactly zero" depends on it)
    for u, v, excl in ((-1.0, 1.5, True), (float(w), 2.5, True), (-1.5, 2.5, False), (w + 3.5, 2.5, False),
                       (2.5, -1.0, True), (2.5, float(h), True), (2.5, -2.25, False), (2.5, h + 2.5, False)):
        add("outside", u, v, excl)
    for u, v in ((w - 0.5, 2.25), (w + 0.5, 2.25), (w + 2.0, 2.25), (2.25, h - 0.5), (2.25, h + 1.0)):
        add("camgrid", u, v)
    zf = 2.0 ** -9                                                                                  # in front, d u / d x = 512
    for u, v in ((1.5, 1.25), (4.75, 3.5)):                                                         # (nothing but the lattice
        q.append(("clamp", u * zf, v * zf, zf, (u, v), False))                                      # point touches token (yi, xi))
    q.append(("clamp", 0.0, 0.0, 2.0 ** -11, (0.0, 0.0), True))                                     # clamped, on the principal point
    for x, y in ((0.5e-3, 0.625e-3), (0.75e-3, 0.375e-3)):                                          # clamped, off the lattice:
        xs, ys = float(np.float32(x / 8)) * 8, float(np.float32(y / 8)) * 8                         # u = x / eps ~ 0.5: generic
        q.append(("clamp", xs, ys, 2.0 ** -11, None, False))
    for x, y, z in ((1.0, -2.0, -1.0), (1000.0, 500.0, -0.5), (-250.0, 3.0, -2.0)):                 # behind: |u| = 1e3 .. 1e6
        q.append(("clamp", x, y, z, (x / EPS, y / EPS), False))
    for u, v in ((-0.5, 1.75), (3.25, -0.125)):
        add("novalid", u, v)
    for u, v in ((1.5, 1.25), (1.5, 1.25)):                                                        # the first clamp query's footprint
        add("pileup", u, v)
    for u, v in ((1.75, 3.125), (4.5, 2.75), (3.375, 0.5), (1.25, 1.875), (1.5, 3.75), (4.125, 1.5)):
        add("generic", u, v)
    return q


def _generic(seed, name, n, T_cl, cam, h, w, region_of):
    """n float32 reference points of ONE scene (T_cl (V,12), cam (V,6)), drawn from seeded uniforms in the view-0 pixel box that
    region_of(i) gives for the i-th query (ulo, uhi, vlo, vhi), depth 0.5 .. 2, keeping those that stay MARGIN away from every
    lattice line in every view, 1e-4 away from the depth clamp, and whose view-0 footprint does not touch token (0, 0)."""
    cand = synth.uniform(seed, name, (64 * n + 256, 3)).astype(np.float64)
    out, k = [], 0
    for i in range(n):
        ulo, uhi, vlo, vhi = region_of(i)
        while True:
            c = cand[k]
            k += 1
            z = 0.5 + 1.5 * c[2]
            r = np.array([(ulo + (uhi - ulo) * c[0]) * z / 8, (vlo + (vhi - vlo) * c[1]) * z / 8, z / 8]).astype(np.float32)
            p2d, zz, _ = project(r[None, None], T_cl[None], cam[None])
            fx0, fy0, on = footprint(p2d[0, 0, 0], h, w)
            if lattice_distance(p2d).min() > MARGIN and np.abs(zz - EPS).min() > 1e-4 and not (on and fx0 <= 0 and fy0 <= 0):
                out.append(r)
                break
    return np.stack(out)


def _round_tokens(a, kind):
    if kind == "f16":
        return a.astype(np.float16).astype(np.float32)
    if kind == "bf16":                                                       # round to nearest even on the upper 16 bits
        b = a.view(np.uint32).astype(np.uint64)
        return (((b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000).astype(np.uint32)).view(np.float32)
    return a


_CACHE = {}


def make_case(cid):
    """dict: B V h w C Q, tok_type, tokens (B, V*h*w, C) float32 holding values of the token type, T_cl (B,V,12) float64, camera
    (B,V,6), ref (B,Q,3), g_tgt (B,Q,C), family (B,Q) str, gref_excluded (B,Q), exact (B,Q), intended (B,Q,2) (NaN where not exact)."""
    if cid in _CACHE:
        return _CACHE[cid]
    B, V, h, w, C, Q, kind = SHAPES[cid]
    seed = 700 + CASE_IDS.index(cid)
    whole = (-1.5, w + 0.5, -1.5, h + 0.5)
    family = np.full((B, Q), "generic", dtype=object)
    excl = np.zeros((B, Q), bool)
    intended = np.full((B, Q, 2), np.nan)
    if cid == "edges":
        T, cam = _poses(seed, B, V, h, w, 1), _camera(B, V, h, w, big_view=1)
        T[0] = IDENTITY                                                      # scene 0: placed queries, identity views only
        placed = _edges_placed(h, w)
        assert len(placed) == Q
        ref = np.zeros((B, Q, 3), np.float32)
        for i, (fam, x, y, z, uv, ex) in enumerate(placed):
            ref[0, i], family[0, i], excl[0, i] = _ref_of(x, y, z), fam, ex
            if uv is not None:
                intended[0, i] = uv
        ref[1] = _generic(seed, "ref", Q, T[1], cam[1], h, w, lambda i: whole)      # scene 1: generic, mixed
    elif cid in ("seams", "chunks"):
        # every 4th query straddles a tile seam (x0 in {7, 15}, y0 = 7, the ragged last tiles), so that every wave of every
        # compaction round and every chunk has hits in every tile; in `chunks` another quarter piles up on a 2 x 2 pixel patch
        T, cam = _poses(seed, B, V, h, w, 1), _camera(B, V, h, w)
        seam = [(7.0, 8.0, -1.0, h + 0.0), (15.0, 17.0, -1.0, h + 0.0), (-1.0, w + 0.0, 7.0, 9.0), (15.0, 17.0, 7.0, 9.0)]
        pile = (7.0, 9.0, 6.0, 8.0)
        region_of = lambda i: seam[(i // 4) % 4] if i % 4 == 3 else pile if (cid == "chunks" and i % 4 == 1) else whole
        ref = _generic(seed, "ref", Q, T[0], cam[0], h, w, region_of)[None]
        family[0, 3::4] = "pileup"
        if cid == "chunks":
            family[0, 1::4] = "pileup"
    else:
        big = 1 if cid.startswith("tok16") else None
        T, cam = _poses(seed, B, V, h, w, 2 if cid.startswith("tok16") else 1), _camera(B, V, h, w, big_view=big)
        ref = _generic(seed, "ref", Q, T[0], cam[0], h, w, lambda i: whole)[None]
    tokens = _round_tokens(synth.normal(seed, "tokens", (B, V * h * w, C)), kind)
    case = dict(id=cid, B=B, V=V, h=h, w=w, C=C, Q=Q, tok_type=("f32", "f16", "bf16").index(kind), tok_kind=kind, tokens=tokens,
                T_cl=np.ascontiguousarray(T), camera=cam, ref=np.ascontiguousarray(ref), g_tgt=synth.normal(seed, "g_tgt", (B, Q, C)),
                family=family, gref_excluded=excl, exact=~np.isnan(intended[..., 0]), intended=intended)
    _CACHE[cid] = case
    return case


def prefill(shape, salt):
    """A non-zero float32 pattern, |value| in [2^-10, 1.5 * 2^-10), signs mixed.  Small against the contributions (|g| ~ 1, weights
    >= MARGIN^2) on purpose: the atomics form rounds once per added term at the magnitude of prefill + partial sum, and the bound of
    the token gradient grants ulp(prefill) once."""
    n = int(np.prod(shape))
    i = np.arange(n, dtype=np.int64)
    mant = 1.0 + ((i * 2654435761 + salt * 40503) % 4096) / 8192.0
    return (np.where(i % 3 == 0, -1.0, 1.0) * mant * 2.0 ** -10).astype(np.float32).reshape(shape)


# ------------------------------------------------------------------------------------------------------------------ float64 oracle
def oracle(case, reference_ops=False):
    """float64 autograd of oracle.parq_oracle.project_and_sample with respect to the tokens and ref, for the loss sum(tgt * g_tgt).
    Returns dict: tgt (B,Q,C), g_tokens (B,N,C), g_ref (B,Q,3), p2d (B,V,Q,2), valid (B,V,Q), jac (B,V,Q,2,3) = d p2d / d ref."""
    import torch
    from oracle import parq_oracle as O
    tok = torch.from_numpy(case["tokens"]).double().requires_grad_()
    ref = torch.from_numpy(case["ref"]).double().requires_grad_()
    T, cam = torch.from_numpy(case["T_cl"]), torch.from_numpy(case["camera"]).double()
    tgt, p2d, valid = O.project_and_sample(tok, O.denormalize(ref, SCALE), T, cam, case["h"], case["w"], reference_ops)
    g_tok, g_ref = torch.autograd.grad((tgt * torch.from_numpy(case["g_tgt"]).double()).sum(), (tok, ref), retain_graph=True)
    jac = torch.zeros(p2d.shape + (3,), dtype=torch.float64)
    for v in range(case["V"]):                       # a query's pixel coordinates depend on its own ref only: one pass per (view, axis)
        for a in range(2):
            jac[:, v, :, a, :] = torch.autograd.grad(p2d[:, v, :, a].sum(), ref, retain_graph=True)[0]
    return dict(tgt=tgt.detach().numpy(), g_tokens=g_tok.numpy(), g_ref=g_ref.numpy(), p2d=p2d.detach().numpy(),
                valid=valid.numpy(), jac=jac.numpy())


def scatter_terms(case, p2d, valid):
    """The scatter of the backward spelled out in float64, term by term, with |.| beside each term:
      g_tokens (B,N,C) the sum of the contributions t_i, abs (B,N,C) the sum of |t_i|, K (B,N) their number (zero weights not counted),
      fwd_abs (B,Q,C) = sum |token * weight| / denom of the forward, Su / Sv (B,V,Q) the absolute sums of the coordinate gradient's
      channel reductions, on (B,V,Q) whether the view samples, stray (list of (b, token)) the stand-in rows of masked corners."""
    B, V, h, w, C, Q = (case[k] for k in ("B", "V", "h", "w", "C", "Q"))
    g, tok = case["g_tgt"].astype(np.float64), case["tokens"].astype(np.float64)
    denom = np.maximum(valid.sum(1), 1).astype(np.float64)                                    # (B,Q)
    fx0, fy0, on = footprint(p2d, h, w)
    out = dict(g_tokens=np.zeros((B, V * h * w, C)), abs=np.zeros((B, V * h * w, C)), K=np.zeros((B, V * h * w), np.int64),
               fwd_abs=np.zeros((B, Q, C)), Su=np.zeros((B, V, Q)), Sv=np.zeros((B, V, Q)), on=on, denom=denom, stray=[])
    for b in range(B):
        for v in range(V):
            u, vv = p2d[b, v, :, 0], p2d[b, v, :, 1]
            for dy in (0, 1):
                for dx in (0, 1):
                    xx, yy = fx0[b, v] + dx, fy0[b, v] + dy
                    inr = (xx >= 0) & (xx <= w - 1) & (yy >= 0) & (yy <= h - 1)
                    ok = on[b, v] & inr
                    wx, wy = 1 - np.abs(u - xx), 1 - np.abs(vv - yy)
                    qs = np.nonzero(ok)[0]
                    rows = v * h * w + (yy[qs] * w + xx[qs]).astype(np.int64)
                    t = g[b, qs] * (wy[qs] * wx[qs] / denom[b, qs])[:, None]
                    np.add.at(out["g_tokens"][b], rows, t)
                    np.add.at(out["abs"][b], rows, np.abs(t))
                    np.add.at(out["K"][b], rows, (wy[qs] * wx[qs] != 0).astype(np.int64))
                    a = np.abs(tok[b, rows])
                    out["fwd_abs"][b, qs] += a * (wy[qs] * wx[qs] / denom[b, qs])[:, None]
                    ga = (np.abs(g[b, qs]) * a).sum(-1) / denom[b, qs]
                    out["Su"][b, v, qs] += ga * wy[qs]
                    out["Sv"][b, v, qs] += ga * wx[qs]
                    for qq in np.nonzero(on[b, v] & ~inr)[0]:                                 # the kernel addresses index 0 instead
                        sx = xx[qq] if 0 <= xx[qq] <= w - 1 else 0
                        sy = yy[qq] if 0 <= yy[qq] <= h - 1 else 0
                        out["stray"].append((b, v * h * w + int(sy * w + sx)))
    return out


def ulp32(a):
    return np.spacing(np.abs(np.asarray(a, np.float32))).astype(np.float64)


def token_bound(terms, pre):
    """|got - want| <= (K + 6) 2^-23 sum|t_i| + ulp(prefill): at most 6 float32 roundings per contribution (1 / denom, the product by
    g, the two weights, the two weight products), (K - 1) 2^-24 sum|t| for a sum of K terms in any order, a factor 2 of slack."""
    return (terms["K"][..., None] + 6) * 2.0 ** -23 * terms["abs"] + ulp32(pre)


def ref_bound(case, terms, jac, pre):
    """|got - want| <= (C / 64 + 14) 2^-23 sum_v (Su_v |du_v / dref_j| + Sv_v |dv_v / dref_j|) + ulp(prefill): the absolute-sum bound
    of the lane-strided float32 sums and the 6-step shuffle tree."""
    s = (terms["Su"][..., None] * np.abs(jac[..., 0, :]) + terms["Sv"][..., None] * np.abs(jac[..., 1, :])).sum(1)      # (B,Q,3)
    return (case["C"] / 64 + 14) * 2.0 ** -23 * s + ulp32(pre)


ORACLE_NOISE = 1e-14          # the float64 oracle's own error: its round trip through the normalised grid turns u = -1 into -1 + 2e-16
#                               when w - 1 is no power of two, a weight of 2e-16 where the exact weight is zero


def forward_bound(case, terms):
    """(4 V + 6) 2^-23 sum|token * weight| / denom per element of tgt: per view four products by a weight that carries three roundings
    and four additions, the cross-view sum and the division."""
    return (4 * case["V"] + 6) * 2.0 ** -23 * terms["fwd_abs"] + ORACLE_NOISE


def unit_rows(case, p2d, terms):
    """(b, token row, q) wherever a query on an exact pixel is the only contribution of that token: one term, weight exactly 1."""
    h, w = case["h"], case["w"]
    u, v = p2d[..., 0], p2d[..., 1]
    hit = (u == np.floor(u)) & (v == np.floor(v)) & (u >= 0) & (u <= w - 1) & (v >= 0) & (v <= h - 1)
    out = []
    for b, vi, q in zip(*np.nonzero(hit)):
        row = vi * h * w + int(v[b, vi, q]) * w + int(u[b, vi, q])
        if terms["K"][b, row] == 1:
            out.append((int(b), int(row), int(q)))
    return out


def tile_hits(case, p2d, first_query):
    """Per (scene, view, 8 x 8 tile): how many queries >= first_query the deterministic gather lists for the tile, (B, V, tiles)."""
    h, w = case["h"], case["w"]
    fx0, fy0, on = footprint(p2d, h, w)
    tx, ty = -(-w // TILE), -(-h // TILE)
    hits = np.zeros((case["B"], case["V"], ty * tx), np.int64)
    for t in range(ty * tx):
        px0, py0 = (t % tx) * TILE, (t // tx) * TILE
        hit = on & (fx0 + 1 >= px0) & (fx0 < px0 + TILE) & (fy0 + 1 >= py0) & (fy0 < py0 + TILE)
        hits[:, :, t] = hit[:, :, first_query:].sum(-1)
    return hits


def wave_hits(case, p2d):
    """Per (scene, view, tile, wave): hits of the first compaction round's four waves (queries 0..255 in 64s)."""
    h, w = case["h"], case["w"]
    fx0, fy0, on = footprint(p2d, h, w)
    tx, ty = -(-w // TILE), -(-h // TILE)
    out = np.zeros((case["B"], case["V"], ty * tx, 4), np.int64)
    for t in range(ty * tx):
        px0, py0 = (t % tx) * TILE, (t // tx) * TILE
        hit = on & (fx0 + 1 >= px0) & (fx0 < px0 + TILE) & (fy0 + 1 >= py0) & (fy0 < py0 + TILE)
        for k in range(4):
            out[:, :, t, k] = hit[:, :, 64 * k:64 * k + 64].sum(-1)
    return out


_ORACLE = {}


def reference(cid):
    """(case, oracle, scatter terms) of a case, computed once and shared (callers do not modify them)."""
    if cid not in _ORACLE:
        case = make_case(cid)
        o = oracle(case)
        _ORACLE[cid] = (case, o, scatter_terms(case, o["p2d"], o["valid"]))
    return _ORACLE[cid]

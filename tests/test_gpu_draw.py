"""GPU tier of the box drawing: parq_draw_boxes (csrc/draw.hip) through parq_amd.draw_boxes against the NumPy statement of the
rule in tests/draw_cases.py, pixel for pixel and bit for bit — box pixels and base pixels alike.  The oracle itself is pinned to
hand-written pixel sets in tests/test_draw_cpu.py.  The raster kernel's tile is 64 x 16 pixels (kTileW x kTileH) and it walks a
view's 12 * M edge slots in chunks of kChunk = 1024."""
import ctypes as C

import numpy as np
import pytest
import torch

from parq_amd import synth
from parq_amd.draw import box_colors, draw_boxes

import draw_cases as D
from gpu_util import dev, lib, sptr

pytestmark = pytest.mark.gpu

NSEM = 9
COLORS = box_colors(NSEM)


def run(sc, keep=None, count=None, uint8=False, with_boxes=True):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    B = sc["images"].shape[0]
    corners = sc["corners"] if with_boxes else np.zeros((B, 0, 8, 3), np.float32)
    labels = sc["labels"] if with_boxes else np.zeros((B, 0), np.int32)
    out = draw_boxes(t(sc["images"]), t(sc["camera"]), t(sc["T_cp"]), t(sc["T_wp"]), t(corners), t(labels),
                     None if keep is None or not with_boxes else t(np.asarray(keep)), None if count is None or not with_boxes else t(np.asarray(count)),
                     num_semcls=NSEM, dtype=torch.uint8 if uint8 else torch.float32)
    return out.cpu().numpy()


def want(sc, keep=None, count=None, uint8=False):
    return D.draw_oracle(sc["images"], sc["camera"], sc["T_cp"], sc["T_wp"], sc["corners"], sc["labels"], keep, count, COLORS, NSEM + 1, uint8)


def same_bits(a, b):
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    if a.dtype == np.float32:
        assert not np.isnan(b).any()
        a, b = a.view(np.uint32), b.view(np.uint32)
    bad = np.argwhere(a != b)
    assert bad.size == 0, "%d of %d values differ, first at %s" % (len(bad), a.size, bad[0])


def check(sc, keep=None, count=None):
    ref, covered = want(sc, keep, count)
    same_bits(run(sc, keep, count), ref)
    return ref, covered


# ------------------------------------------------------------------ hand case

def test_frontal_box_covers_the_hand_written_outline():
    sc = D.lattice_scene(9, 12, [D.flat_box(2, 2, 8, 6)], [3])
    literal = D.art(["............",
                     "..#######...",
                     ".#########..",
                     ".#########..",
                     ".###...###..",
                     ".#########..",
                     ".#########..",
                     "..#######...",
                     "............"])
    got, base = run(sc), run(sc, with_boxes=False)
    covered = np.any(got[0] != base[0], axis=0)
    assert np.array_equal(covered, literal)
    assert np.array_equal(got[0][:, literal], np.repeat(COLORS[3][:, None], literal.sum(), axis=1))
    same_bits(base[0], D.normalise(sc["images"][0, 0]))


# ------------------------------------------------------------------ random cases

@pytest.mark.parametrize("seed", [7101, 7102])
def test_random_scenes_equal_the_oracle_on_every_pixel(seed):
    sc, st = D.random_scene(seed)
    assert st["rejected"] <= 0.20 * st["tried"]
    _, covered = check(sc, keep=sc["keep"])
    assert covered.any() and not covered.all()
    check(sc)                                                             # keep = None: every non-background box


# ------------------------------------------------------------------ tile seams

@pytest.mark.parametrize("hw", [(9, 70), (9, 130), (20, 70), (33, 130)], ids=lambda s: "%dx%d" % s)
def test_edges_across_tile_seams(hw):
    """The tile is 64 wide, as the mandated 9 x 70 and 9 x 130 cases assume: edges cross x = 63 / 64 and 127 / 128.  It is 16 high,
    not 4, so the edges along and across a tile's last row are in the added 20 x 70 and 33 x 130 cases (rows 15 / 16 and 31 / 32)."""
    H, W = hw
    boxes = [D.flat_box(60, 2, 67, 6), D.flat_box(63, 1, 64, 7), D.flat_box(2, 0, 63, 3), D.flat_box(64, 4, 69, 8)]
    if W > 128:
        boxes += [D.flat_box(120, 1, 129, 7), D.flat_box(127, 0, 128, 8), D.flat_box(1, 5, 127, 6)]
    if H > 16:
        boxes += [D.flat_box(10, 15, 50, 18), D.flat_box(5, 12, 66, 16), D.flat_box(30, 3, 33, 15), D.flat_box(61, 14, 66, 17)]
    if H > 32:
        boxes += [D.flat_box(100, 31, 129, 32), D.flat_box(20, 16, 90, 31)]
    boxes = np.concatenate([np.stack(boxes), D.random_lattice_boxes(H * 1000 + W, 6, 0, W - 1, 0, H - 1)])
    labels = np.arange(len(boxes)) % NSEM
    sc = D.lattice_scene(H, W, boxes, labels, seed=W)
    _, covered = check(sc)
    assert covered[0, :, 63].any() and covered[0, :, 64].any()


# ------------------------------------------------------------------ chunking

def test_four_hundred_boxes_across_one_tile_keep_their_order_through_the_chunks():
    """M = 400 boxes = 4800 slots, all of whose edges lie inside tile (0, 0): more than 4 x kChunk (1024) kept entries for that
    tile, walked in five chunks.  Classes alternate, so a chunk taken in the wrong order shows."""
    M = 400
    assert M * 12 >= 4 * D.CHUNK
    boxes = D.random_lattice_boxes(77, M, 0, D.TILE_W - 1, 0, D.TILE_H - 1)
    sc = D.lattice_scene(20, 70, boxes, np.arange(M) % 2 * 5 + np.arange(M) % 3)
    check(sc)
    thin = D.lattice_scene(20, 70, np.stack([D.flat_box(3 + (m % 50), 2 + (m % 7), 8 + (m % 50), 6 + (m % 9)) for m in range(M)]),
                           np.arange(M) % 2, seed=5)
    check(thin)


# ------------------------------------------------------------------ validity

def _segments(sc):
    return D.view_segments(sc["camera"][0, 0], sc["T_cp"][0, 0], sc["T_wp"][0, 0], sc["corners"][0], sc["labels"][0], None, None, NSEM + 1)


def test_a_corner_behind_the_camera_takes_its_three_edges_with_it():
    box = D.lattice_box([(2, 2), (9, 1), (10, 6), (3, 7), (4, 3), (7, 3), (7, 5), (4, 5)])
    box[0, 2] = -2.0
    sc = D.lattice_scene(9, 12, [box], [1])
    segs = _segments(sc)
    assert len(segs) == 9 and all((2, 2) not in ((s[0], s[1]), (s[2], s[3])) for s in segs)
    check(sc)


def test_a_corner_on_the_last_column_is_drawn_and_half_a_pixel_beyond_is_not():
    H, W = 9, 12
    on = D.lattice_scene(H, W, [D.flat_box(4, 2, W - 1, 6)], [2])
    assert len(_segments(on)) == 12
    _, covered = check(on)
    assert covered[0, 2:7, W - 1].all()
    box = D.flat_box(4, 2, W - 1, 6)
    box[1, 0] = box[5, 0] = W - 0.5                                        # corners 1 and 5: u = w - 0.5 > w - 1
    off = D.lattice_scene(H, W, [box], [2])
    u, _, _, valid = D.project(off["camera"][0, 0], off["T_cp"][0, 0], off["T_wp"][0, 0], box)
    assert u[1] == W - 0.5 and not valid[1] and not valid[5] and valid[[0, 2, 3, 4, 6, 7]].all()
    assert len(_segments(off)) == 12 - 5                                  # 01, 12, 15, 45, 56 go
    _, covered = check(off)
    assert not covered[0, 0:2, 6:].any()                                  # nothing of the top edge 01


def test_a_corner_exactly_on_the_near_plane_is_not_in_front():
    """z = 1e-3 as a float64, reached as the left-to-right sum of three float32 terms through a T_camera_pseudoCam whose third
    row adds x to z (the rule is stated on the arithmetic; the matrix need not be a rotation).  One float32 ulp more in the middle
    term and the corner is in front."""
    hi, mid, lo = D.exact_depth_split(1e-3)
    for bump, front in ((False, False), (True, True)):
        m = np.nextafter(mid, np.float32(1.0)) if bump else mid
        pts = np.array([(m, 0, hi), (1, 0, 2), (1, 1, 2), (0, 1, 2), (0, -1, 2), (1, -1, 2), (1, 2, 2), (0, 2, 2)], np.float32)
        sc = D.lattice_scene(9, 12, [pts], [4])
        sc["camera"][0, 0] = [12, 9, 2, 2, 5, 4]
        sc["T_cp"][0, 0] = [1, 0, 0, 0, 1, 0, 1, 0, 1, 0, 0, lo]
        u, v, z, valid = D.project(sc["camera"][0, 0], sc["T_cp"][0, 0], sc["T_wp"][0, 0], pts)
        assert (z[0] == 1e-3) == (not front) and (z[0] > 1e-3) == front and bool(valid[0]) == front
        assert 0 <= u[0] <= 11 and 0 <= v[0] <= 8 and valid[1:].all()
        assert len(_segments(sc)) == (12 if front else 9)
        check(sc)


# ------------------------------------------------------------------ order

def _two_scene_case():
    a, b = D.flat_box(2, 2, 12, 8), D.flat_box(6, 4, 18, 11)
    pad = D.flat_box(20, 1, 30, 5)
    other = [D.flat_box(24, 6, 36, 12), D.flat_box(1, 10, 9, 13), D.flat_box(33, 0, 39, 3)]
    boxes = np.stack([np.stack([a, b, pad]), np.stack(other)])
    labels = np.array([[0, 5, 7], [2, 3, 8]], np.int32)
    return D.lattice_scene(15, 41, boxes, labels, B=2, T=2, seed=11)


def test_the_later_box_wins_keep_and_count_remove_boxes():
    sc = _two_scene_case()
    ref, _ = check(sc)
    assert np.array_equal(ref[0][:, 4, 6:13], np.repeat(COLORS[5][:, None], 7, axis=1))         # box 1's top edge over box 0's right side
    keep = np.array([[1, 0, 1], [1, 1, 1]], bool)
    ref_k, _ = check(sc, keep=keep)
    assert np.array_equal(ref_k[0][:, 4, 11:14], np.repeat(COLORS[0][:, None], 3, axis=1))      # box 0's right edge shows again
    count = np.array([2, 1], np.int32)
    ref_c, covered = check(sc, count=count)
    assert not covered[0, 0:7, 22:32].any() and not covered[1, 0:4, 32:].any()                  # the padded boxes are gone
    check(sc, keep=keep, count=count)


def test_scenes_do_not_mix_and_the_batch_equals_each_scene_alone():
    sc = _two_scene_case()
    both = run(sc)
    for b in (0, 1):
        alone = {k: v[b:b + 1] for k, v in sc.items()}
        same_bits(run(alone), both[b:b + 1])
    only0 = dict(sc, labels=np.stack([sc["labels"][0], np.full(3, NSEM, np.int32)]))            # scene 1 all background
    got = run(only0)
    same_bits(got[0], both[0])
    same_bits(got[1], run(sc, with_boxes=False)[1])
    swapped = dict(sc, corners=sc["corners"][::-1].copy(), labels=sc["labels"][::-1].copy())
    assert not np.array_equal(run(swapped)[0], both[0])                                         # scene 0 draws its own boxes


# ------------------------------------------------------------------ normalisation

@pytest.mark.parametrize("hw", [(23, 41), (7, 5), (1, 1), (64, 67)], ids=lambda s: "%dx%d" % s)
def test_normalisation_is_bit_equal_to_float32_numpy(hw):
    H, W = hw
    rng = np.random.default_rng(H * 100 + W)
    images = (rng.standard_normal((2, 3, 3, H, W)) * rng.uniform(0.1, 50.0, (2, 3, 1, 1, 1)) + rng.uniform(-5, 5, (2, 3, 1, 1, 1))).astype(np.float32)
    sc = D.lattice_scene(H, W, np.zeros((0, 8, 3), np.float32), np.zeros(0, np.int32), B=2, T=3, images=images)
    got = run(sc, with_boxes=False)
    for b in range(2):
        for t in range(3):
            same_bits(got[b][:, t * H:(t + 1) * H], D.normalise(images[b, t]))
    same_bits(run(sc, uint8=True, with_boxes=False), D.to_uint8(got))


def test_a_nan_pixel_makes_its_view_nan_except_under_a_box_and_a_constant_view_is_nan():
    sc = D.lattice_scene(9, 12, [D.flat_box(2, 2, 8, 6)], [3], B=1, T=3, seed=3)
    sc["images"][0, 0, 1, 4, 5] = np.nan
    sc["images"][0, 1] = 0.25
    got = run(sc)
    ref, covered = want(sc)
    assert np.array_equal(got, ref, equal_nan=True)
    v0, v1, v2 = got[0][:, 0:9], got[0][:, 9:18], got[0][:, 18:27]
    box = covered[0, 0:9]
    assert box.sum() == 56
    for v in (v0, v1):
        assert np.isnan(v[:, ~box]).all()
        assert np.array_equal(v[:, box], np.repeat(COLORS[3][:, None], 56, axis=1))
    assert not np.isnan(v2).any()
    u8 = run(sc, uint8=True)
    assert np.array_equal(u8, D.to_uint8(ref)) and (u8[0][:, 0:9][:, ~box] == 0).all()


def test_uint8_output_is_numpys_truncation():
    sc, _ = D.random_scene(7103)
    ref, _ = want(sc, keep=sc["keep"])
    got = run(sc, keep=sc["keep"], uint8=True)
    assert got.dtype == np.uint8
    same_bits(got, (ref * np.float32(255.0)).astype(np.uint8))
    same_bits(got, want(sc, keep=sc["keep"], uint8=True)[0])
    assert {tuple(r) for r in np.trunc(COLORS * np.float32(255.0)).astype(np.uint8).tolist()} >= {(153, 61, 61), (229, 91, 91)}


def test_out_argument_and_wrappers():
    from parq_amd import Camera, Pose
    sc, _ = D.random_scene(7104)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    B, T, _, H, W = sc["images"].shape
    out = torch.full((B, 3, T * H, W), -3.0, device="cuda")
    res = draw_boxes(t(sc["images"]), Camera(t(sc["camera"])), Pose(t(sc["T_cp"])), Pose(t(sc["T_wp"]).double()), t(sc["corners"]),
                     t(sc["labels"]).long(), t(sc["keep"]), num_semcls=NSEM, out=out)
    assert res is out
    same_bits(out.cpu().numpy(), want(sc, keep=sc["keep"])[0])


# ------------------------------------------------------------------ argument errors

def test_bad_arguments_are_refused_and_write_nothing():
    l = lib()
    B, T, H, W, M = 1, 2, 6, 8, 3
    img, cam, pose = torch.zeros(B, T, 3, H, W, device="cuda"), torch.zeros(B, T, 6, device="cuda"), torch.zeros(B, T, 12, device="cuda")
    cw, lab = torch.zeros(B, M, 8, 3, device="cuda"), torch.zeros(B, M, dtype=torch.int32, device="cuda")
    col = torch.from_numpy(COLORS).cuda()
    need = l.parq_draw_boxes_workspace_bytes(B, T, M)
    ws = torch.full((need // 4 + 4,), 5.0, device="cuda")
    out = torch.full((B, 3, T * H, W), 7.0, device="cuda")
    p = lambda x: C.c_void_p(x.data_ptr())
    good = dict(images=p(img), camera=p(cam), T_cp=p(pose), T_wp=p(pose), corners=p(cw), labels=p(lab), keep=None, count=None, colors=p(col),
                ncls=NSEM + 1, B=B, T=T, H=H, W=W, M=M, ws=p(ws), ws_bytes=need, out=p(out), u8=0)
    order = ("images", "camera", "T_cp", "T_wp", "corners", "labels", "keep", "count", "colors", "ncls", "B", "T", "H", "W", "M", "ws", "ws_bytes",
             "out", "u8")
    call = lambda **kw: l.parq_draw_boxes(*[dict(good, **kw)[k] for k in order], sptr())
    bad = [dict(images=None), dict(camera=None), dict(T_cp=None), dict(T_wp=None), dict(ws=None), dict(out=None), dict(corners=None),
           dict(labels=None), dict(colors=None), dict(ws_bytes=need - 1), dict(ws_bytes=0), dict(H=8193), dict(W=8193), dict(B=0), dict(M=-1),
           dict(u8=2), dict(ncls=1)]
    for kw in bad:
        assert call(**kw) == 1, kw                                         # PARQ_ERR_ARG
        assert l.parq_last_error().decode().startswith("parq_draw_boxes"), kw
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((ws == 5.0).all())
    assert call(M=0, corners=None, labels=None, colors=None) == 0          # M = 0 is valid: the normalised image
    assert call() == 0
    torch.cuda.synchronize()
    assert not bool((out == 7.0).any())


def test_python_checks_run_on_gpu_tensors_too():
    sc = D.lattice_scene(9, 12, [D.flat_box(2, 2, 8, 6)], [3])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    with pytest.raises(ValueError, match="is on cpu"):
        draw_boxes(t(sc["images"]), t(sc["camera"]), t(sc["T_cp"]), t(sc["T_wp"]), torch.from_numpy(sc["corners"]), t(sc["labels"]), num_semcls=NSEM)
    with pytest.raises(ValueError, match="labels must be"):
        draw_boxes(t(sc["images"]), t(sc["camera"]), t(sc["T_cp"]), t(sc["T_wp"]), t(sc["corners"]), t(sc["labels"])[:, :0], num_semcls=NSEM)


# ------------------------------------------------------------------ module

def _module_case():
    from types import SimpleNamespace as NS
    from parq_amd import PARQ
    B, V, H, W = 2, 2, 24, 32
    dcfg = synth.decoder_cfg(dim=128, queries=32, heads=2, ffn=96, layers=2)
    dcfg.FOR_VIS = True
    cfg = NS(MODEL=NS(TOKENIZER=NS(OUT_CHANNELS=128, RAY_POINTS_SCALE=dcfg.TRANSFORMER.SCALE, NUM_SAMPLES=64, MIN_DEPTH=0.25, MAX_DEPTH=5.25),
                      DECODER=dcfg))
    model = PARQ(cfg).eval()
    Wd = synth.make_decoder_weights(dcfg, 7201)
    sd = model.state_dict()
    for k in sd:
        if k.startswith("box3d_decoder."):
            sd[k] = torch.from_numpy(Wd[k[len("box3d_decoder."):].replace("parq_module.decoder.mlp_heads.", "mlp_heads.")]).reshape(sd[k].shape)
    model.load_state_dict(sd, strict=True)
    model = model.cuda()
    scn = synth.make_scene(7202, B=B, V=V, h=8, w=8, C=128)
    cam, T_cp, T_wp, T_wl = (dev(a) for a in synth.make_geometry(7202, B, V, H, W))             # the same poses, cameras at image size
    with torch.no_grad():
        outputs = model.box3d_decoder(dev(scn["tokens"]), dev(scn["camera"]), T_cp, T_wp, T_wl)
    obbs, _ = synth.make_boxes(7203, B, 5, max_box=8)
    # ground truth box 0 of scene 0: 3 m in front of view 0 (pseudo-camera frame), so that at least one box is inside an image
    R, tw = T_wp[0, 0, :9].reshape(3, 3).cpu().numpy(), T_wp[0, 0, 9:].cpu().numpy()
    obbs[0, 0, 15:18] = R @ np.array([0.0, 0.0, 3.0], np.float32) + tw
    obbs[0, 0, 0:6] = [-0.3, 0.3, -0.3, 0.3, -0.3, 0.3]
    batch = {"rgb_img": dev(synth.normal(7204, "rgb", (B, V, 3, H, W))), "camera": cam, "T_camera_pseudoCam": T_cp, "T_world_pseudoCam": T_wp,
             "T_world_local": T_wl, "obbs_padded": dev(obbs), "scene_name": ["scene0000_00", "scene0001_00"], "snippet_id": torch.tensor([12])}
    return model, batch, outputs, (B, V, H, W)


def test_log_images_equals_draw_boxes_on_parse_preds_boxes_and_mask(tmp_path):
    from parq_amd.wrappers import Obb3D, Pose, raw
    model, batch, outputs, (B, V, H, W) = _module_case()
    dec = model.box3d_decoder
    args = (outputs, batch["obbs_padded"], batch["T_world_pseudoCam"], batch["T_world_local"], batch["T_camera_pseudoCam"], batch["rgb_img"],
            batch["camera"])
    assert dec.log_images(*args) == {}                                    # the flag is off by default
    assert model.get_log_images(batch, outputs) == {}
    dec.draw_images = True
    ims = dec.log_images(*args)
    assert sorted(ims) == ["rgb_img", "rgb_img_gtwithbox", "rgb_imgwithbox"]
    for v in ims.values():
        assert v.is_cuda and v.dtype == torch.float32 and tuple(v.shape) == (3, V * H, W)
    out = dec.parse_pred(outputs)
    obbs, mask = out["obbs_pred"], out["pred_mask"]
    corners = Pose(batch["T_world_local"]).transform(obbs.T_world_object.transform(obbs.bb3corners_object))
    view = (batch["rgb_img"][0:1], batch["camera"][0:1], batch["T_camera_pseudoCam"][0:1], batch["T_world_pseudoCam"][0:1])
    pred = draw_boxes(*view, corners[0:1], raw(obbs)[0:1, :, 18].int(), keep=mask[0:1], num_semcls=NSEM)
    assert torch.equal(ims["rgb_imgwithbox"], pred[0])
    base = np.concatenate([D.normalise(batch["rgb_img"][0, t].cpu().numpy()) for t in range(V)], axis=1)
    same_bits(ims["rgb_img"].cpu().numpy(), base)
    gt = Obb3D(batch["obbs_padded"][0:1, :5])                             # up to its padding, no mask
    gtw = draw_boxes(*view, gt.T_world_object.transform(gt.bb3corners_object), raw(gt)[..., 18].int(), num_semcls=NSEM)
    assert torch.equal(ims["rgb_img_gtwithbox"], gtw[0])
    assert not torch.equal(ims["rgb_img_gtwithbox"], ims["rgb_img"])      # the box placed in front of view 0 is drawn
    assert sorted(dec.log_images(outputs, None, *args[2:])) == ["rgb_img", "rgb_imgwithbox"]
    # PARQ: the same overlays as uint8 NumPy arrays, and PNG files under the reference's name rule
    arrs = model.get_log_images(batch, outputs)
    assert sorted(arrs) == sorted(ims)
    for tag, a in arrs.items():
        assert isinstance(a, np.ndarray) and a.dtype == np.uint8 and a.shape == (3, V * H, W)
        same_bits(a, D.to_uint8(ims[tag].cpu().numpy()))
    import importlib.util
    if importlib.util.find_spec("PIL") is not None:                       # (the PNG writer itself: tests/test_draw_cpu.py)
        paths = model.vis_output(batch, outputs, output_name=str(tmp_path / "demo"))
        assert sorted(p.split("/")[-1] for p in paths) == ["scene0000_00_12_%s.png" % tag for tag in sorted(ims)]

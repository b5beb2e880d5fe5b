"""CPU tier of the box drawing (parq_amd/draw.py, include/parq_hip.h parq_draw_boxes): the NumPy statement of the rule
(tests/draw_cases.py) against covered pixel sets written out by hand — these literals are the authority, the oracle is checked
against them and the kernel against the oracle —, the colour table, the argument checks, the entry points' declaration and
binding, the PNG writer and the random generator's rejection share."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import parq_amd
from parq_amd import _lib
from parq_amd.draw import box_colors, check_draw_args, draw_boxes

import draw_cases as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_horizontal_segment_covers_three_rows_and_two_end_caps():
    want = np.zeros((9, 12), bool)
    want[2:5, 2:7] = True                      # rows 2-4 x columns 2-6
    want[3, 1] = want[3, 7] = True             # (1, 3) and (7, 3)
    assert np.array_equal(D.segment_cover(9, 12, 2, 3, 6, 3), want)
    assert np.array_equal(D.segment_cover(9, 12, 6, 3, 2, 3), want)


def test_diagonal_segment():
    want = D.art(["............",
                  "..#.........",
                  ".###........",
                  "..###.......",
                  "...###......",
                  "....###.....",
                  ".....#......",
                  "............",
                  "............"])
    assert np.array_equal(D.segment_cover(9, 12, 2, 2, 5, 5), want)
    assert np.array_equal(D.segment_cover(9, 12, 5, 5, 2, 2), want)


def test_zero_length_segment_is_a_plus():
    want = np.zeros((9, 12), bool)
    for x, y in ((4, 4), (3, 4), (5, 4), (4, 3), (4, 5)):
        want[y, x] = True
    assert np.array_equal(D.segment_cover(9, 12, 4, 4, 4, 4), want)
    corner = np.zeros((9, 12), bool)
    corner[0, 0] = corner[0, 1] = corner[1, 0] = True
    assert np.array_equal(D.segment_cover(9, 12, 0, 0, 0, 0), corner)      # clipped by the image


def test_the_later_of_two_overlapping_colours_wins():
    cls = D.paint(9, 12, [(2, 3, 6, 3, 0), (4, 1, 4, 6, 1)])
    later = np.zeros((9, 12), bool)
    later[1:7, 3:6] = True                     # columns 3-5 x rows 1-6
    later[0, 4] = later[7, 4] = True
    earlier_only = np.zeros((9, 12), bool)
    earlier_only[2:5, 2] = earlier_only[2:5, 6] = True
    earlier_only[3, 1] = earlier_only[3, 7] = True
    assert np.array_equal(cls == 1, later)
    assert np.array_equal(cls == 0, earlier_only)
    assert np.array_equal(cls == -1, ~(later | earlier_only))


FLAT_BOX_ART = ["............",
                "..#######...",
                ".#########..",
                ".#########..",
                ".###...###..",
                ".#########..",
                ".#########..",
                "..#######...",
                "............"]


def test_oracle_draws_a_frontal_box_as_the_hand_written_outline():
    sc = D.lattice_scene(9, 12, [D.flat_box(2, 2, 8, 6)], [3])
    colors = box_colors(9)
    out, covered = D.draw_oracle(sc["images"], sc["camera"], sc["T_cp"], sc["T_wp"], sc["corners"], sc["labels"], None, None, colors, 10)
    want = D.art(FLAT_BOX_ART)
    assert np.array_equal(covered[0], want)
    assert np.array_equal(out[0][:, want], np.repeat(colors[3][:, None], want.sum(), axis=1))
    assert np.array_equal(out[0][:, ~want], D.normalise(sc["images"][0, 0])[:, ~want])


def test_box_colors():
    c = box_colors(9)
    assert c.shape == (9, 3) and c.dtype == np.float32
    want = np.array([(0.6, 0.24, 0.24), (0.9, 0.36, 0.36), (0.24, 0.6, 0.6), (0.36, 0.9, 0.9)], np.float32)
    assert np.array_equal(c[:4], want)
    assert len({tuple(r) for r in c.tolist()}) == 9
    assert box_colors(0).shape == (0, 3)
    assert np.array_equal(box_colors(20)[:9], c)
    assert parq_amd.box_colors is box_colors and parq_amd.draw_boxes is draw_boxes


def _args(B=2, T=3, H=5, W=7, M=4):
    return dict(images=torch.zeros(B, T, 3, H, W), camera=torch.zeros(B, T, 6), T_camera_pseudoCam=torch.zeros(B, T, 12),
                T_world_pseudoCam=torch.zeros(B, T, 12), corners_world=torch.zeros(B, M, 8, 3), labels=torch.zeros(B, M, dtype=torch.int64),
                keep=None, count=None, num_semcls=9, dtype=torch.float32, out=None)


def test_argument_errors_are_value_errors_before_the_gpu():
    _, dims = check_draw_args(**_args())
    assert dims == (2, 3, 5, 7, 4)
    from parq_amd import Camera, Pose
    a = _args()
    a.update(camera=Camera(a["camera"]), T_world_pseudoCam=Pose(a["T_world_pseudoCam"]), keep=torch.ones(2, 4, dtype=torch.bool),
             count=torch.tensor([4, 2]))
    assert check_draw_args(**a)[1] == dims                                           # the project's wrappers pass
    for key, bad, match in (
            ("images", torch.zeros(2, 3, 1, 5, 7), "images must be"), ("images", torch.zeros(2, 3, 3, 5, 7, dtype=torch.float64), "float32"),
            ("images", torch.zeros(1, 1, 3, 8193, 2), "at most"), ("camera", torch.zeros(2, 3, 5), "camera must be"),
            ("T_camera_pseudoCam", torch.zeros(2, 2, 12), "T_camera_pseudoCam must be"),
            ("T_world_pseudoCam", torch.zeros(2, 3, 12, dtype=torch.int32), "floating-point"),
            ("corners_world", torch.zeros(2, 4, 8, 2), "corners_world must be"), ("corners_world", torch.zeros(1, 4, 8, 3), "corners_world must be"),
            ("labels", torch.zeros(2, 5, dtype=torch.int64), "labels must be"), ("labels", torch.zeros(2, 4), "integer"),
            ("keep", torch.zeros(2, 3, dtype=torch.bool), "keep must be"), ("keep", torch.zeros(2, 4), "bool or uint8"),
            ("count", torch.zeros(3, dtype=torch.int64), "count must be"), ("count", torch.zeros(2), "integer"),
            ("num_semcls", 0, "num_semcls"), ("num_semcls", True, "num_semcls"), ("dtype", torch.float16, "dtype must be"),
            ("out", torch.zeros(2, 3, 15, 7, dtype=torch.uint8), "out must be"), ("out", torch.zeros(2, 3, 5, 7), "out must be")):
        a = _args()
        a[key] = bad
        with pytest.raises(ValueError, match=match):
            check_draw_args(**a)


def test_cpu_tensors_are_a_runtime_error_there_is_no_cpu_path():
    a = _args()
    pos = [a.pop(k) for k in ("images", "camera", "T_camera_pseudoCam", "T_world_pseudoCam", "corners_world", "labels")]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        draw_boxes(*pos, **a)


def test_header_declares_both_entry_points_and_the_binding_types_them():
    hdr = open(os.path.join(ROOT, "include", "parq_hip.h")).read()
    m = re.search(r"\bint\s+\(?parq_draw_boxes\)?\s*\(([^;]*)\)\s*;", hdr)
    assert m, "include/parq_hip.h must declare parq_draw_boxes"
    params = [p.strip() for p in re.sub(r"/\*.*?\*/", "", m.group(1).replace("\n", " ")).split(",")]
    assert [p.split()[-1].lstrip("*") for p in params] == [
        "images", "camera", "T_camera_pseudoCam", "T_world_pseudoCam", "corners_world", "labels", "keep", "count", "colors", "num_classes",
        "B", "T", "H", "W", "M", "workspace", "workspace_bytes", "out", "out_uint8", "stream"]
    assert re.search(r"\bsize_t\s+\(?parq_draw_boxes_workspace_bytes\)?\s*\(\s*int32_t B,\s*int32_t T,\s*int32_t M\s*\)\s*;", hdr)
    for name in ("parq_draw_boxes", "parq_draw_boxes_workspace_bytes"):
        assert name in _lib.EXTRA_SYMBOLS and name not in _lib.SYMBOLS
    res, args = _lib.EXTRA_SYMBOLS["parq_draw_boxes"]
    assert res is C.c_int and len(args) == len(params)
    assert args[9:15] == [C.c_int32] * 6 and args[16] is C.c_size_t and args[18] is C.c_int32
    assert _lib.EXTRA_SYMBOLS["parq_draw_boxes_workspace_bytes"] == (C.c_size_t, [C.c_int32] * 3)


def test_library_exports_and_types_both_entry_points():
    lib = _lib.load()
    for name in ("parq_draw_boxes", "parq_draw_boxes_workspace_bytes"):
        fn = getattr(lib, name)
        assert fn.argtypes == _lib.EXTRA_SYMBOLS[name][1] and fn.restype is _lib.EXTRA_SYMBOLS[name][0]
    per_view = lib.parq_draw_boxes_workspace_bytes(1, 1, 0)
    assert per_view > 0 and per_view % 16 == 0
    assert lib.parq_draw_boxes_workspace_bytes(2, 3, 5) == 6 * per_view + 2 * 3 * 5 * 12 * 8
    assert lib.parq_draw_boxes_workspace_bytes(0, 1, 1) == 0 and lib.parq_draw_boxes_workspace_bytes(1, 1, -1) == 0


def test_save_log_images_round_trip(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    from parq_amd.module import PARQ
    rng = np.random.default_rng(3)
    ims = {"rgb_img": rng.integers(0, 256, (3, 10, 7), dtype=np.uint8), "rgb_imgwithbox": rng.integers(0, 256, (3, 10, 7), dtype=np.uint8)}
    paths = PARQ.save_log_images(ims, str(tmp_path / "vis" / "deep"), "scene0000_00_12")
    assert sorted(os.path.basename(p) for p in paths) == ["scene0000_00_12_rgb_img.png", "scene0000_00_12_rgb_imgwithbox.png"]
    for tag, im in ims.items():
        back = np.asarray(Image.open(str(tmp_path / "vis" / "deep" / ("scene0000_00_12_%s.png" % tag))))
        assert back.shape == (10, 7, 3) and np.array_equal(back.transpose(2, 0, 1), im)


def test_log_images_and_get_log_images_return_nothing_while_the_flag_is_off():
    from types import SimpleNamespace as NS
    from parq_amd import synth
    from parq_amd.decoder import PARQDecoder
    from parq_amd.module import PARQ
    assert PARQDecoder.draw_images is False
    dcfg = synth.decoder_cfg(dim=128, queries=32, heads=2, ffn=256, layers=1)
    cfg = NS(MODEL=NS(TOKENIZER=NS(OUT_CHANNELS=128, RAY_POINTS_SCALE=dcfg.TRANSFORMER.SCALE, NUM_SAMPLES=64, MIN_DEPTH=0.25, MAX_DEPTH=5.25),
                      DECODER=dcfg))
    model = PARQ(cfg)
    assert model.box3d_decoder.log_images([], None, None, None, None, rgb_img=torch.zeros(1, 1, 3, 4, 4)) == {}
    assert model.get_log_images({"rgb_img": torch.zeros(1, 1, 3, 4, 4)}, []) == {}
    for name in ("get_log_images", "save_log_images", "vis_output"):
        assert callable(getattr(PARQ, name))


def test_random_generator_rejects_at_most_a_fifth_of_its_boxes():
    tried = rejected = boxes = drawable = 0
    for seed in (7101, 7102, 7103, 7104):
        _, st = D.random_scene(seed)
        tried, rejected, boxes, drawable = tried + st["tried"], rejected + st["rejected"], boxes + st["boxes"], drawable + st["drawable"]
    print("rejected %d of %d sampled boxes; %d of %d kept boxes have a drawable edge" % (rejected, tried, drawable, boxes))
    assert rejected <= 0.20 * tried
    assert drawable >= 0.8 * boxes

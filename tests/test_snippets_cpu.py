"""CPU tier of the snippet targets (parq_amd/snippets.py; include/parq_hip.h parq_snippet_targets): the NumPy statement of the rule
(tests/snippet_cases.py) against what the reference's own functions gave (tests/golden/g25_snippets.npz, written by
tools/make_golden_snippets.py), ``select_views`` against the reference's four frame selections, the argument checks, and the
header / binding / export agreement."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import torch

import snippet_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Z, META = SC.load_golden()
IDS = [c["name"] for c in SC.CASES]
_statement = {}


def statement(c):
    if c["name"] not in _statement:
        res = SC.case_statement(c)
        for v in res.values():
            v.setflags(write=False)
        _statement[c["name"]] = res
    return _statement[c["name"]]


def test_the_fixture_is_of_these_cases():
    assert META["cases"] == json.loads(json.dumps(SC.CASES))
    assert os.path.getsize(SC.GOLDEN) < 1 << 20


@pytest.mark.parametrize("c", SC.CASES, ids=IDS)
def test_statement_gives_the_reference_counts_levels_and_rows_exactly(c):
    got, p = statement(c), c["name"] + "/"
    for key in ("frame_points", "points_inside", "difficulty", "valid", "num_valid"):
        assert got[key].shape == Z[p + key].shape and np.array_equal(got[key], Z[p + key]), key
    assert got["obbs_padded"].dtype == np.float32 and np.array_equal(got["obbs_padded"].view(np.uint32), Z[p + "obbs_padded"].view(np.uint32))
    assert got["sym"].dtype == Z[p + "sym"].dtype and np.array_equal(got["sym"], Z[p + "sym"])
    for b in range(c["B"]):                                                        # the valid rows, in order, then padding
        rows = SC.make_case(c)["obbs"][b][got["valid"][b]]
        assert np.array_equal(got["obbs_padded"][b, :len(rows)], rows) and np.all(got["obbs_padded"][b, len(rows):] == -1)


@pytest.mark.parametrize("c", SC.CASES, ids=IDS)
def test_statement_ratios_agree_with_the_reference(c):
    got, p = statement(c), c["name"] + "/"
    for key in ("frame_truncation", "truncation"):
        err = SC.parity(got[key], Z[p + key])
        print("%s %s: parity %.3e" % (c["name"], key, err))
        assert got[key].dtype == np.float32 and err <= 1e-4


def test_the_cases_reach_what_they_name():
    lv = statement(SC.case_by_name("levels_96x128"))
    assert set(lv["difficulty"][0].tolist()) == {0, 1, 2, 3}
    pts = lv["points_inside"]
    for thr, _ in SC.DEFAULT_LEVELS:
        assert (pts[pts > 0] < thr).any() and (pts > thr).any()
    assert lv["num_valid"].tolist() == [int(v.sum()) for v in lv["valid"]] and lv["num_valid"][0] != lv["num_valid"][1]
    assert 61 * 77 % 4 == 1 and 61 * 77 > 2 * SC.TILE_PIXELS                        # an odd frame length over three tiles
    pad = statement(SC.case_by_name("n1_and_padding"))
    assert pad["points_inside"][1].tolist() == [0] and pad["num_valid"].tolist() == [0, 0]
    zero = statement(SC.case_by_name("zero_frame"))
    assert not zero["frame_points"][0, 0].any() and zero["frame_points"][0, 1].any()
    clamp = statement(SC.case_by_name("clamp_t1"))
    assert clamp["points_inside"][0, 0] > 1000 and clamp["difficulty"][0, 0] == 3   # encloses the camera: every point, a tiny ratio
    assert clamp["truncation"][0, 2] == 0 and clamp["truncation"][0, 3] == 0        # outside the image, behind the camera
    assert statement(SC.case_by_name("nothing_valid"))["num_valid"].tolist() == [0]
    d = SC.make_case(SC.case_by_name("six_digits"))
    R = d["T_world_camera"][0, :, :3, :3]
    off = np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max()
    assert 1e-8 < off < 1e-5                                                        # orthonormal to six digits, not further
    assert np.any(d["corners_world"] != d["corners_world"].astype(np.float32))


@pytest.mark.parametrize("v", SC.LEVEL_VARIANTS, ids=[v["case"] for v in SC.LEVEL_VARIANTS])
def test_other_thresholds_and_max_box(v):
    c = SC.case_by_name(v["case"])
    base = statement(c)
    got = SC.case_statement(c, levels=v["levels"], max_level=v["max_level"], max_box=v["max_box"])
    assert np.array_equal(got["points_inside"], base["points_inside"]) and np.array_equal(got["truncation"], base["truncation"])
    assert got["obbs_padded"].shape[1] == v["max_box"]
    want = [[SC.level_of(p, r, v["levels"]) for p, r in zip(P, R)] for P, R in zip(base["points_inside"], base["truncation"])]
    assert got["difficulty"].tolist() == want
    assert got["num_valid"].tolist() == [min(int(x.sum()), v["max_box"]) for x in got["valid"]]
    if v["case"] == "n128_32x40":
        assert got["valid"].sum() > v["max_box"]                                    # rows beyond max_box are dropped


def test_the_inverse_is_general_not_the_transpose():
    M = np.eye(4)
    M[:3, :3] = [[1.0, 0.2, 0.0], [0.0, 1.0, 0.0], [0.1, 0.0, 2.0]]
    M[:3, 3] = [0.5, -1.0, 2.0]
    Ri, ti = SC.affine_inverse(M)
    inv = np.linalg.inv(M)
    assert np.allclose(Ri, inv[:3, :3], rtol=0, atol=1e-15) and np.allclose(ti, inv[:3, 3], rtol=0, atol=1e-15)
    assert not np.allclose(Ri, M[:3, :3].T)


# ---- select_views ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(3))
def test_select_views_gives_the_reference_id_lists(i):
    from parq_amd import select_views
    g = META["select"][i]
    kw = dict(window_size=g["window_size"], min_angle=g["min_angle"], min_distance=g["min_distance"])
    traj = SC.make_trajectory()
    for mode in ("val", "w1", "train", "all"):
        got = select_views(traj, mode, **kw)
        assert got == g[mode], (mode, kw)
        assert all(isinstance(v, int) for ids in got for v in ids)
    as_dict = {i_: M for i_, M in enumerate(traj) if np.isfinite(M).all()}
    assert select_views(as_dict, "train", **kw) == g["train"]
    assert select_views(torch.from_numpy(traj), "val", **kw) == g["val"]
    assert g["all"][0] and g["train"] and (g["val"] or g["window_size"] == 1)


def test_select_views_argument_errors():
    from parq_amd import select_views
    traj = SC.make_trajectory()
    for bad in (dict(mode="test"), dict(window_size=0), dict(window_size=2.0), dict(min_angle="15"), dict(min_distance=None)):
        kw = dict(mode="val")
        kw.update(bad)
        with pytest.raises(ValueError, match="select_views"):
            select_views(traj, **kw)
    with pytest.raises(ValueError, match="select_views"):
        select_views(traj[:, :3], "val")
    with pytest.raises(ValueError, match="select_views"):
        select_views({0.5: np.eye(4)}, "val")
    assert select_views(np.full((3, 4, 4), np.inf), "all") == [[]]


# ---- SnippetTargets: argument errors before anything touches the GPU ---------------------------------------------------------------
def _inputs():
    d = SC.make_case(SC.case_by_name("zero_frame"))
    t = {k: torch.from_numpy(v) for k, v in d.items() if isinstance(v, np.ndarray)}
    return [t["depth"], t["depth_intrinsics"], t["color_intrinsics"], d["color_size"], t["T_world_camera"], t["obbs"], t["sym"]]


def test_snippet_targets_argument_errors():
    from parq_amd import SnippetTargets
    for kw in (dict(levels=()), dict(levels=((1, 0.5),) * 9), dict(levels=((1.5, 0.5),)), dict(levels=((-1, 0.5),)), dict(levels=((1, "a"),)),
               dict(levels=[(5, 0.5, 1)]), dict(max_level=4), dict(max_level=-1), dict(max_level=1.0), dict(depth_scale=0),
               dict(depth_scale=float("inf")), dict(depth_scale="mm"), dict(max_box=0), dict(max_box=2.5)):
        with pytest.raises(ValueError, match="SnippetTargets"):
            SnippetTargets(**kw)
    tg = SnippetTargets()
    assert tg.levels == SC.DEFAULT_LEVELS and tg.max_level == 3 and tg.depth_scale == 1000.0 and tg.max_box == 100
    good = _inputs()
    bad = {0: [good[0].to(torch.int32), good[0][0], good[0][:, :, ::2], good[0].to(torch.int16), None],
           1: [good[1][0, :2], good[1].to(torch.int32), torch.zeros(1, 4, 4), good[1].repeat(2, 1, 1)],
           2: [good[2][0, :, :2], good[2].repeat(3, 1, 1)],
           3: [(64,), (0, 80), (64, 8193), (64.0, 80), None],
           4: [good[4][:, :1], good[4].to(torch.int64), good[4][..., :3, :]],
           5: [good[5].double(), good[5][..., :18], good[5][0], good[5].repeat(2, 1, 1), torch.zeros(1, 129, 19), torch.zeros(1, 0, 19)],
           6: [good[6].double(), good[6][0], good[6].repeat(2, 1), good[6][:, :0], None]}
    for i, values in bad.items():
        for v in values:
            a = list(good)
            a[i] = v
            with pytest.raises(ValueError, match="SnippetTargets"):
                tg(*a)
    for cw in (torch.zeros(1, 5, 8, 2), torch.zeros(1, 4, 8, 3), torch.zeros(1, 5, 8, 3, dtype=torch.int32), np.zeros((1, 5, 8, 3))):
        with pytest.raises(ValueError, match="corners_world"):
            tg(*good, corners_world=cw)
    with pytest.raises(ValueError, match="at most"):
        tg(torch.zeros(1, 65, 2, 2, dtype=torch.uint16), *good[1:])
    with pytest.raises(RuntimeError, match="no CPU"):                                # all arguments fine, the depth on the CPU
        tg(*good)


# ---- header, binding, exports ---------------------------------------------------------------------------------------------------
def test_header_declares_the_two_entry_points_and_the_binding_types_them():
    from parq_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "parq_hip.h")).read()
    want = {"parq_snippet_targets_workspace": ["B", "T", "Hd", "Wd", "N"],
            "parq_snippet_targets": ["depth", "B", "T", "Hd", "Wd", "depth_intrinsics_inv", "color_intrinsics", "color_h", "color_w",
                                     "T_world_camera", "obbs", "corners_world", "sym", "sym_is_int", "S", "N", "max_box",
                                     "level_counts_host", "level_ratios_host", "n_levels", "max_level", "depth_scale", "workspace",
                                     "workspace_bytes", "obbs_padded", "sym_out", "num_valid", "frame_points", "frame_truncation",
                                     "points_inside", "truncation", "difficulty", "valid", "stream"]}
    for name, names in want.items():
        m = re.search(r"\b(?:int|size_t)\s+\(%s\)\s*\(([^;]*)\)\s*;" % name, hdr)
        assert m, "include/parq_hip.h must declare %s" % name
        params = [p.strip() for p in re.sub(r"/\*.*?\*/", "", m.group(1).replace("\n", " ")).split(",")]
        assert [p.split()[-1].lstrip("*") for p in params] == names, name
        assert name in _lib.SNIPPET_SYMBOLS and name not in _lib.SYMBOLS and name not in _lib.EXTRA_SYMBOLS
        res, args = _lib.SNIPPET_SYMBOLS[name]
        assert len(args) == len(names) and res is (C.c_size_t if name.endswith("workspace") else C.c_int)
    assert sum(len(t) for t in _lib.ALL_TABLES) == 92 and len(_lib.SNIPPET_SYMBOLS) == 2
    assert re.search(r"\b89\b", open(os.path.join(ROOT, "README.md")).read())
    for doc, word in (("INTEGRATION.md", "## Targets from depth"), ("tools/README.md", "make_golden_snippets.py"),
                      ("tools/README.md", "snippet_targets_time.py")):
        assert word in open(os.path.join(ROOT, doc)).read(), (doc, word)


def test_library_exports_the_entry_points_and_sizes():
    from parq_amd import _lib
    lib = _lib.load()
    for name, (res, args) in _lib.SNIPPET_SYMBOLS.items():
        fn = getattr(lib, name)
        assert fn.argtypes == args and fn.restype is res
    size = lib.parq_snippet_targets_workspace
    assert size(2, 3, 96, 128, 24) == 2 * 3 * 7 * 24 * 4                            # 12288 pixels (+ 3): 7 tiles of 2048
    assert size(1, 1, 1, 1, 1) == 16 and size(4, 3, 480, 640, 40) == 4 * 3 * 151 * 40 * 4
    for bad in ((0, 1, 8, 8, 1), (1024, 1, 8, 8, 1), (1, 0, 8, 8, 1), (1, 65, 8, 8, 1), (1, 1, 0, 8, 1), (1, 1, 8, 8193, 1), (1, 1, 8193, 8, 1),
                (1, 1, 8, 8, 0), (1, 1, 8, 8, 129), (-1, 1, 8, 8, 1)):
        assert size(*bad) == 0, bad
    assert size(1023, 64, 8192, 8192, 128) > 2 ** 32                                # no 32-bit overflow at the limits


def test_the_package_exports_the_names_lazily():
    import parq_amd
    from parq_amd import snippets
    assert parq_amd.SnippetTargets is snippets.SnippetTargets and parq_amd.select_views is snippets.select_views
    src = open(os.path.join(ROOT, "parq_amd", "csrc", "snippets.hip")).read()
    assert "#pragma clang fp contract(off)" in src and "atomic" not in src.lower().replace("no atomics", "")
    res = open(os.path.join(ROOT, "profiles", "snippet_targets_kernel_resources.txt")).read()
    assert res.count("ScratchSize [bytes/lane]: 0") == 2 and "snippet_count_kernel" in res and "snippet_finalize_kernel" in res

"""CPU tier of the frame preparation (parq_amd/frames.py, include/parq_hip.h parq_frame_plan / parq_frames_resize): the NumPy
statement of the resize rule (tests/frames_cases.py) against the bytes the reference's own transforms produced
(tests/golden/g24_frames.npz) and, where Pillow is installed, against Pillow itself; the host plan function against the statement's
plan integer for integer; the declarations and bindings; the argument checks; intrinsics and poses against the fixture."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import parq_amd
from parq_amd import Pose, _lib
from parq_amd import frames as F

import frames_cases as FC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Z, META = FC.load_golden()
RESIZE_IDS = [c["name"] for c in FC.RESIZE_CASES]
POSE_IDS = [c["name"] for c in FC.POSE_CASES]
_statement = {}


def statement(c):
    """The statement's bytes of a case, computed once and shared."""
    if c["name"] not in _statement:
        res = FC.resize_statement(FC.case_frames(c), FC.pad4(c["pad"], c["inp"]), tuple(c["out"]))
        res.setflags(write=False)
        _statement[c["name"]] = res
    return _statement[c["name"]]


def test_fixture_was_made_from_these_cases():
    norm = lambda cases: [{k: (list(v) if isinstance(v, tuple) else v) for k, v in c.items()} for c in cases]
    assert META["resize"] == norm(FC.RESIZE_CASES) and META["poses"] == norm(FC.POSE_CASES)
    assert os.path.getsize(FC.GOLDEN) < 1024 * 1024


@pytest.mark.parametrize("c", FC.RESIZE_CASES, ids=RESIZE_IDS)
def test_statement_equals_the_reference_bytes(c):
    want = Z[c["name"] + "/bytes"]
    got = statement(c)
    assert got.dtype == np.uint8 and got.shape == want.shape == (c["n"], 3, c["out"][1], c["out"][0])
    assert np.array_equal(got, want)


def test_statement_equals_the_reference_bytes_of_the_two_scene_case():
    c = FC.POSE_CASES[2]
    got = FC.resize_statement(FC.case_frames(c), FC.pad4(c["pad"], c["inp"]), tuple(c["out"]))
    assert np.array_equal(got.reshape(Z[c["name"] + "/bytes"].shape), Z[c["name"] + "/bytes"])


@pytest.mark.parametrize("c", FC.RESIZE_CASES, ids=RESIZE_IDS)
def test_statement_equals_pillow(c):
    Image = pytest.importorskip("PIL.Image")
    ImageOps = pytest.importorskip("PIL.ImageOps")
    pad = FC.pad4(c["pad"], c["inp"])
    for f, want in zip(FC.case_frames(c), statement(c)):
        im = Image.fromarray(f, "RGB")
        if any(pad):
            im = ImageOps.expand(im, border=pad)
        got = np.array(im.resize(tuple(c["out"]), Image.BILINEAR))
        assert np.array_equal(got.transpose(2, 0, 1), want)


def test_white_stays_white_and_black_black():
    c = next(c for c in FC.RESIZE_CASES if c["name"] == "white_black")
    res = statement(c)
    assert (res[0] == 255).all() and (res[1] == 0).all()


def _axes():
    seen = []
    for c in FC.RESIZE_CASES + FC.POSE_CASES:
        l, t, r, b = FC.pad4(c["pad"], c["inp"])
        for pair in ((c["inp"][0] + l + r, c["out"][0]), (c["inp"][1] + t + b, c["out"][1])):
            if pair not in seen:
                seen.append(pair)
    return seen


@pytest.mark.parametrize("inp,out", _axes(), ids=["%d_to_%d" % p for p in _axes()])
def test_host_plan_equals_the_statements_plan(inp, out):
    want = FC.plan_ints(inp, out)
    lib = _lib.load()
    assert lib.parq_frame_plan_ints(inp, out) == want.size == 1 + out * (2 + want[0])
    got = np.full(want.size + 2, -7, np.int32)                    # two guard words behind the plan
    assert lib.parq_frame_plan(inp, out, got.ctypes.data_as(C.POINTER(C.c_int32))) == 0
    assert np.array_equal(got[:-2], want) and (got[-2:] == -7).all()
    assert np.array_equal(F.frame_plan(inp, out), want)


def test_identity_axis_plan_is_the_identity():
    ksize, xmin, n, k = FC.axis_plan(16, 16)
    assert ksize == 3
    for xx in range(16):
        taps = {int(xmin[xx] + x): int(k[xx, x]) for x in range(n[xx]) if k[xx, x]}
        assert taps == {xx: 4194304}


def test_plan_sums_keep_the_accumulator_inside_int32():
    for inp, out in _axes():
        _, _, _, k = FC.axis_plan(inp, out)
        assert (k >= 0).all() and int(k.sum(1).max()) * 255 + 2097152 < 2 ** 31


def test_plan_ints_refuses_what_the_header_documents():
    lib = _lib.load()
    assert lib.parq_frame_plan_ints(64, 8) == 1 + 8 * (2 + 17)                    # 8x: the largest downscale, 17 taps
    assert lib.parq_frame_plan_ints(8192, 8192) == 1 + 8192 * 5
    assert lib.parq_frame_plan_ints(1, 8192) > 0                                  # upscaling is not limited
    for inp, out in ((65, 8), (0, 8), (8, 0), (-3, 8), (8, -1), (8193, 8192), (8192, 8193)):
        assert lib.parq_frame_plan_ints(inp, out) == 0, (inp, out)
        buf = np.full(4, -7, np.int32)
        assert lib.parq_frame_plan(inp, out, buf.ctypes.data_as(C.POINTER(C.c_int32))) == 1      # PARQ_ERR_ARG
        assert (buf == -7).all()
        with pytest.raises(ValueError):
            F.frame_plan(inp, out)
    assert lib.parq_frame_plan(16, 16, None) == 1


def test_header_declares_the_three_entry_points_and_the_binding_types_them():
    hdr = open(os.path.join(ROOT, "include", "parq_hip.h")).read()
    names = {"parq_frame_plan_ints": ("size_t", ["in_size", "out_size"]),
             "parq_frame_plan": ("int", ["in_size", "out_size", "plan_host"]),
             "parq_frames_resize": ("int", ["frames", "N", "H_in", "W_in", "pad_left", "pad_top", "pad_right", "pad_bottom", "plan_x",
                                            "plan_y", "H_out", "W_out", "out", "out_uint8", "stream"])}
    for name, (res, params) in names.items():
        m = re.search(r"\b%s\s+\(%s\)\s*\(([^;]*)\)\s*;" % (res, name), hdr)
        assert m, "include/parq_hip.h must declare %s with a parenthesised name" % name
        got = [p.strip().split()[-1].lstrip("*") for p in m.group(1).replace("\n", " ").split(",")]
        assert got == params
        assert name in _lib.EXTRA_SYMBOLS and name not in _lib.SYMBOLS
        assert len(_lib.EXTRA_SYMBOLS[name][1]) == len(params)
    assert _lib.EXTRA_SYMBOLS["parq_frame_plan_ints"] == (C.c_size_t, [C.c_int32] * 2)
    assert _lib.EXTRA_SYMBOLS["parq_frame_plan"] == (C.c_int, [C.c_int32, C.c_int32, C.POINTER(C.c_int32)])
    res, args = _lib.EXTRA_SYMBOLS["parq_frames_resize"]
    assert res is C.c_int and args[1:8] == [C.c_int32] * 7 and args[10:12] == [C.c_int32] * 2 and args[13] is C.c_int32
    lib = _lib.load()
    for name in names:
        fn = getattr(lib, name)
        assert fn.argtypes == _lib.EXTRA_SYMBOLS[name][1] and fn.restype is _lib.EXTRA_SYMBOLS[name][0]


def test_lazy_exports():
    for name in ("resize_frames", "resized_intrinsics", "gravity_aligned", "snippet_local", "FramePrep"):
        assert getattr(parq_amd, name) is getattr(F, name)


def test_argument_errors_are_value_errors_before_the_gpu():
    fr = torch.zeros(2, 3, 37, 53, 3, dtype=torch.uint8)
    lead, hw, wh, pad = F.check_frames_args(fr, (16, 12), "scannet", torch.float32, None)
    assert (lead, tuple(hw), wh, pad) == ((2, 3), (37, 53), (16, 12), (0, 0, 0, 0))
    assert F.check_frames_args(torch.zeros(968, 1296, 3, dtype=torch.uint8), (320, 240), "scannet", torch.uint8, None)[3] == (0, 2, 0, 2)
    bad = [dict(frames=fr.float()), dict(frames=fr[..., :2]), dict(frames=fr[:, :, :, ::2]), dict(frames=fr[0, 0, 0]),
           dict(frames=np.zeros((37, 53, 3), np.uint8)), dict(frames=torch.zeros(0, 37, 53, 3, dtype=torch.uint8)),
           dict(size=(16,)), dict(size=(16, 0)), dict(size=(16.0, 12)), dict(size=(True, 12)), dict(size=(6, 12)), dict(size=(16, 4)),
           dict(size=(8193, 12)), dict(pad="scan"), dict(pad=(0, 2, 0)), dict(pad=(0, -1, 0, 0)), dict(pad=(0, 2.0, 0, 2)),
           dict(pad=(0, 60, 0, 0)), dict(dtype=torch.float16), dict(out=torch.zeros(2, 3, 3, 12, 16)[..., :15]),
           dict(out=torch.zeros(2, 3, 3, 12, 16, dtype=torch.uint8)), dict(out=torch.zeros(2, 3, 3, 16, 12))]
    for kw in bad:
        a = dict(frames=fr, size=(16, 12), pad="scannet", dtype=torch.float32, out=None)
        a.update(kw)
        with pytest.raises(ValueError):
            F.resize_frames(**a)
    with pytest.raises(ValueError):
        F.resize_frames(torch.zeros(8193, 4, 3, dtype=torch.uint8), (4, 2000), None)


def test_cpu_tensors_are_a_runtime_error_there_is_no_cpu_path():
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        F.resize_frames(torch.zeros(37, 53, 3, dtype=torch.uint8), (16, 12))
    prep = F.FramePrep(size=(16, 12))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        prep(torch.zeros(1, 2, 37, 53, 3, dtype=torch.uint8), torch.eye(3).expand(1, 2, 3, 3), torch.eye(4).expand(1, 2, 4, 4))


def test_frame_prep_and_pose_argument_errors():
    for kw in (dict(size=(16,)), dict(pad="x"), dict(up=(0, 0, 0)), dict(up=(0, 1)), dict(frame_selection=1.0), dict(frame_selection=-0.1)):
        with pytest.raises(ValueError):
            F.FramePrep(**kw)
    prep = F.FramePrep(size=(16, 12))
    fr = torch.zeros(1, 2, 37, 53, 3, dtype=torch.uint8)
    K, M = torch.eye(3).expand(1, 2, 3, 3), torch.eye(4).expand(1, 2, 4, 4)
    for a in ((fr[0], K, M), (fr, K[:, :1], M), (fr, K, M[:, :1]), (fr, K.long(), M), (fr, K, M[..., :3])):
        with pytest.raises(ValueError):
            prep(*a)
    with pytest.raises(ValueError):
        F.gravity_aligned(torch.zeros(2, 3, 4))
    with pytest.raises(ValueError):
        F.snippet_local(torch.zeros(3, 12))
    with pytest.raises(ValueError):
        F.resized_intrinsics(torch.zeros(3, 2), (53, 37), (16, 12), None)


@pytest.mark.parametrize("c", FC.POSE_CASES, ids=POSE_IDS)
def test_resized_intrinsics_are_bit_equal_to_the_fixture(c):
    K, _ = FC.case_poses(c)
    got = F.resized_intrinsics(torch.from_numpy(K), tuple(c["inp"]), tuple(c["out"]), c["pad"])
    assert got.dtype == torch.float32 and got.shape == K.shape
    got = got.numpy()
    want = Z[c["name"] + "/camera"]                                # rows [w, h, fx, fy, cx, cy] of view 0 of each scene
    w, h = c["out"]
    for b in range(c["B"]):
        row = np.array([w, h, got[b, 0, 0, 0], got[b, 0, 1, 1], got[b, 0, 0, 2], got[b, 0, 1, 2]], np.float32)
        for t in range(c["T"]):
            assert np.array_equal(row.view(np.uint32), want[b, t].view(np.uint32))
    assert np.array_equal(got[..., 2, :], np.broadcast_to(np.float32([0, 0, 1]), got[..., 2, :].shape))
    assert np.array_equal(F.resized_intrinsics(K, tuple(c["inp"]), tuple(c["out"]), c["pad"]).numpy(), got)       # arrays are taken too


@pytest.mark.parametrize("c", FC.POSE_CASES, ids=POSE_IDS)
def test_gravity_aligned_and_snippet_local_against_the_fixture(c):
    _, M = FC.case_poses(c)
    bound = FC.pose_bound(M)
    T_wp, T_cp = F.gravity_aligned(torch.from_numpy(M))
    assert isinstance(T_wp, Pose) and isinstance(T_cp, Pose) and T_wp._data.dtype == torch.float32
    p = c["name"] + "/"
    for got, key in ((T_wp, "T_world_pseudoCam"), (T_cp, "T_camera_pseudoCam"), (F.snippet_local(T_wp), "T_world_local")):
        want = Z[p + key]
        err = np.abs(got._data.numpy().astype(np.float64) - want.astype(np.float64)).max()
        print("%s %s: max |a - b| = %.3e, bound %.3e" % (c["name"], key, err, bound))
        assert got._data.shape == want.shape and err <= bound
    want = Z[p + "T_world_pseudoCam"]
    got = T_wp._data.numpy()
    assert np.array_equal(got[..., 9:], want[..., 9:]) and np.array_equal(got[..., 9:], M[..., :3, 3])       # the translation: copied
    assert np.array_equal(got[..., [1, 4, 7]], want[..., [1, 4, 7]])                                            # column 1 = up
    assert np.array_equal(got[..., [1, 4, 7]], np.broadcast_to(np.float32([0, 0, 1]), got[..., :3].shape))
    local = F.snippet_local(T_wp._data)
    t = int(c["T"] * 0.5)
    assert isinstance(local, torch.Tensor) and torch.equal(local, T_wp._data[:, t:t + 1])
    assert local.data_ptr() != T_wp._data[:, t:t + 1].data_ptr()
    assert torch.equal(F.snippet_local(T_wp, 0.0)._data, T_wp._data[:, :1])
    again, _ = F.gravity_aligned(Pose.from_4x4mat(torch.from_numpy(M)))
    assert torch.equal(again._data, T_wp._data)


def test_normalisation_is_per_view_with_one_view_looking_straight_up():
    _, M = FC.case_poses(FC.POSE_CASES[0])
    M = torch.from_numpy(M).clone()
    alone, _ = F.gravity_aligned(M)
    up = M.clone()
    up[0, 1, :3, :3] = torch.tensor([[1.0, 0, 0], [0, -1, 0], [0, 0, -1]]).T @ torch.eye(3)      # forward axis (0, 0, -1): along -up
    up[0, 1, :3, 2] = torch.tensor([0.0, 0, 1])                                                  # ... and straight along up
    T_wp, T_cp = F.gravity_aligned(up)
    R = T_wp.R
    assert torch.equal(R[0, 1, :, 2], torch.zeros(3)) and torch.equal(R[0, 1, :, 0], torch.zeros(3))      # nothing to normalise: left as it is
    assert torch.equal(R[0, 1, :, 1], torch.tensor([0.0, 0, 1]))
    for t in (0, 2):                                                    # the other views are normalised as if the view were not there
        assert torch.equal(T_wp._data[0, t], alone._data[0, t])
        assert abs(float(torch.linalg.norm(R[0, t, :, 2])) - 1) < 1e-6
    assert torch.isfinite(T_wp._data).all() and torch.isfinite(T_cp._data).all()
